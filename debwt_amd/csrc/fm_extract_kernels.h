// fm_extract_kernels.h -- the third query of the FM-index: extract.  The text is read back from the rank lines by LF
// walks that start on sampled rows, as ASCII for (record, offset, length) jobs and as the packed 2-bit text for the
// whole collection (debwt_fm_restore_text).
//
// Anchors.  The samples are row-sampled (sa[i] = position of the suffix in row i * s); extraction needs the nearest known
// (position, row) at or after a text position.  The anchors are the sampled pairs ordered by position, closed at both
// ends by the two pairs every index has for free where no sample holds them: (0, the '$' row) and (n - 1, row n - 1).
// They are kept as a permutation of sample numbers, 8 bytes per sample: perm[k] = i says anchor k is (sa[i], i * s);
// the values nsamp and nsamp + 1 stand for (n - 1, n - 1) and (0, '$' row).  No sort and no packed key, so no capacity
// below the index's own: the sampled positions are marked in a bitmap of n bits (a position >= n or marked twice is
// counted: the samples are refused), a rank over the bitmap (one u32 per word inside chunks of 256 words, one u64 per
// chunk) gives every position its place, and one scatter writes the permutation.  The bitmap and its rank (n / 8 +
// n / 16 bytes) are released after the build.
//
// Walk.  An item is the stretch between two consecutive anchors (or the part of it a job needs): a lane starts on the
// upper anchor's row and takes exactly (upper position - stop position) LF steps, a difference of two checked positions
// below n -- no loop waits for a row, so wrong samples cost wrong letters or a refused chain, never an endless walk or a
// store outside the item's own output range.  Each step is one dependent 128-byte line read, so the kernel lives on
// lanes in flight.  Gaps between row-sampled positions are about geometric with mean s: one item per lane would leave
// most of a wave waiting for its longest gap.  Instead a wave owns a run of `chunk` consecutive items and its lanes take
// the next item of the run whenever they finish one (a wave-uniform counter in a register: no atomics, no LDS); the
// lanes idle only while the last items of the run drain.  steps / wave_steps reports the share of lanes busy.
// Single TU: included by debwt_hip.hip only, after fm_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"

#define FM_EX_CHUNK_WORDS 256           // bitmap words per rank chunk (one workgroup)

// counters of the anchor build
#define FM_EX_A_RANGE 0                 // samples that are no text position
#define FM_EX_A_DUP 1                   // samples on a position another sample holds
#define FM_EX_A_FIRST 2                 // 1: position 0 is not sampled, the free anchor (0, '$' row) was added
#define FM_EX_A_LAST 3                  // 1: position n - 1 is not sampled, the free anchor (n - 1, n - 1) was added
#define FM_EX_A_TOTAL 4                 // set bits of the bitmap (k_fm_anc_scan)
// counters of a walk
#define FM_EX_W_STEPS 0
#define FM_EX_W_WAVE 1                  // 64 x the loop iterations of every wave
#define FM_EX_W_CHAIN 2                 // items that did not arrive on the row of their lower anchor (or, the first, on '$')
#define FM_EX_W_BAD 3                   // items with anchors out of order, rows outside the BWT, a separator inside a job
#define FM_EX_W_SEPS 4                  // separators met by the packed emitter

struct FmAnchors {
    const u64 *perm;       // na sample numbers, ascending by position
    const u64 *sa;
    u64 na, nsamp;
    u32 sh;
};

__device__ __forceinline__ void fm_anchor(const FmAnchors &A, const VIndex &V, u64 k, u64 *pos, u64 *row) {
    const u64 i = A.perm[k];
    if (i < A.nsamp) { *pos = A.sa[i]; *row = i << A.sh; }
    else if (i == A.nsamp) { *pos = V.n - 1; *row = V.n - 1; }
    else { *pos = 0; *row = V.dollar_row; }
}

// ---- anchors ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_fm_anc_mark(const u64 *__restrict__ sa, u64 nsamp, u64 n, u64 *__restrict__ bits,
                                                     u64 *__restrict__ ctr) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsamp) return;
    const u64 p = sa[i];
    if (p >= n) { atomicAdd(&ctr[FM_EX_A_RANGE], 1ull); return; }
    const u64 bit = 1ull << (p & 63);
    if (atomicOr(&bits[p >> 6], bit) & bit) atomicAdd(&ctr[FM_EX_A_DUP], 1ull);
}
// the two free anchors, where no sample holds their position (one thread; n >= 2)
__global__ void k_fm_anc_free(u64 n, u64 *__restrict__ bits, u64 *__restrict__ ctr) {
    if (blockIdx.x || threadIdx.x) return;
    if (!(bits[0] & 1ull)) { bits[0] |= 1ull; ctr[FM_EX_A_FIRST] = 1; }
    const u64 w = (n - 1) >> 6, bit = 1ull << ((n - 1) & 63);
    if (!(bits[w] & bit)) { bits[w] |= bit; ctr[FM_EX_A_LAST] = 1; }
}
// rank, pass 1: set bits before every word inside its chunk, and per chunk
__global__ __launch_bounds__(FM_EX_CHUNK_WORDS) void k_fm_anc_count(const u64 *__restrict__ bits, u64 nwords, u32 *__restrict__ wpre,
                                                                    u64 *__restrict__ csum) {
    __shared__ u32 smem[DEBWT_WAVES + 1];
    const u64 w = (u64)blockIdx.x * FM_EX_CHUNK_WORDS + threadIdx.x;
    const u32 c = w < nwords ? (u32)__popcll(bits[w]) : 0u;
    u32 total;
    const u32 ex = block_scan_excl(c, smem, &total);
    if (w < nwords) wpre[w] = ex;
    if (threadIdx.x == 0) csum[blockIdx.x] = total;
}
// rank, pass 2: exclusive scan of the chunk sums in place (one workgroup); *total = all set bits
__global__ __launch_bounds__(1024) void k_fm_anc_scan(u64 *__restrict__ csum, u64 nchunks, u64 *__restrict__ total) {
    __shared__ u64 part[1024];
    const u32 tid = threadIdx.x;
    const u64 per = (nchunks + 1023) / 1024;
    const u64 lo = (u64)tid * per < nchunks ? (u64)tid * per : nchunks, hi = lo + per < nchunks ? lo + per : nchunks;
    u64 s = 0;
    for (u64 i = lo; i < hi; i++) s += csum[i];
    part[tid] = s;
    __syncthreads();
    for (u32 d = 1; d < 1024; d <<= 1) {
        const u64 v = tid >= d ? part[tid - d] : 0ull;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u64 run = part[tid] - s;
    for (u64 i = lo; i < hi; i++) { const u64 c = csum[i]; csum[i] = run; run += c; }
    if (tid == 1023) *total = part[1023];
}
// the permutation: sample i (and the free anchors, i = nsamp and nsamp + 1, where added) goes to the rank of its
// position.  Only after k_fm_anc_mark counted no position >= n and none twice.
__global__ __launch_bounds__(256) void k_fm_anc_scatter(const u64 *__restrict__ sa, u64 nsamp, u64 n, const u64 *__restrict__ bits,
                                                        const u32 *__restrict__ wpre, const u64 *__restrict__ csum,
                                                        const u64 *__restrict__ ctr, u64 na, u64 *__restrict__ perm) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsamp + 2) return;
    u64 p;
    if (i < nsamp) p = sa[i];
    else if (i == nsamp) { if (!ctr[FM_EX_A_LAST]) return; p = n - 1; }
    else { if (!ctr[FM_EX_A_FIRST]) return; p = 0; }
    if (p >= n) return;
    const u64 w = p >> 6;
    const u64 k = csum[w / FM_EX_CHUNK_WORDS] + wpre[w] + (u64)__popcll(bits[w] & ((1ull << (p & 63)) - 1ull));
    if (k < na) perm[k] = i;
}

// ---- emitters ---------------------------------------------------------------------------------------------------------
// An emitter turns item t into a walk (load) and takes the symbol of every step (emit).  A walk: start on `row`, the
// suffix at position p; every step yields the symbol at p - 1 and moves there; stop when p == stop.  check: the walk
// ends on the lower anchor itself and must arrive on want_row.

struct FmExWalk { u64 p, stop, row, want_row; bool check; };

// Packed text: item t is the gap between anchors t and t + 1, all of it.  Codes are collected per text word and stored
// whole where the word lies inside the gap; the partial words at the two ends are merged into the zeroed buffer with
// atomicOr.  Separators are stored as code 3 and their positions listed for the host ('$' with bit 63 set).
struct FmExPacked {
    u64 *text;             // ((n + 63) >> 5) + 2 words, zeroed
    u64 *seppos;           // sepcap entries
    u64 sepcap;
    struct State { u64 acc, hi; };

    __device__ __forceinline__ bool load(const VIndex &V, const FmAnchors &A, u64 t, FmExWalk *w, State *st) const {
        u64 lp, lr;
        fm_anchor(A, V, t, &lp, &lr);
        fm_anchor(A, V, t + 1, &w->p, &w->row);
        w->stop = lp; w->want_row = lr; w->check = true;
        st->acc = 0; st->hi = w->p;
        bool ok = w->p > lp && w->p < V.n && w->row < V.n;
        if (t == 0 && (lp != 0 || lr != V.dollar_row)) ok = false;     // the text begins on the '$' row
        return ok;
    }
    __device__ __forceinline__ bool emit(const FmExWalk &w, State *st, u64 pos, u32 sym, u64 *ctr) const {
        st->acc |= (u64)(sym > 3 ? 3u : sym) << (2 * (31 - (u32)(pos & 31)));
        if (sym > 3) {
            const u64 slot = atomicAdd(&ctr[FM_EX_W_SEPS], 1ull);
            if (slot < sepcap) seppos[slot] = pos | (sym == 5 ? 1ull << 63 : 0ull);
        }
        if ((pos & 31) == 0 || pos == w.stop) {
            if ((pos & 31) == 0 && pos + 32 <= st->hi) text[pos >> 5] = st->acc;
            else atomicOr(&text[pos >> 5], st->acc);
            st->acc = 0;
        }
        return true;
    }
};

// '$' at position n - 1, which no walk yields (it is the symbol before position 0), and the 32 'T' behind it
// (debwt_load_text's layout); the words behind stay zero
__global__ void k_fm_extract_pad(u64 *__restrict__ text, u64 n) {
    const u64 p = n - 1 + threadIdx.x;
    if (blockIdx.x || threadIdx.x >= 33) return;
    atomicOr(&text[p >> 5], 3ull << (2 * (31 - (u32)(p & 31))));
}

// ASCII: job j covers text positions [a, b) inside one record; its items are the anchor gaps klo .. klo + nseg - 1 that
// meet it, item t of the batch belonging to the last job j with seg0[j] <= t (seg0: njobs + 1 prefix sums of nseg).  The
// part of a gap at or after b is walked but not emitted; the walk stops at a when the lower anchor lies before it.
struct FmExJob { u64 a, b, out, klo; };

struct FmExAscii {
    const FmExJob *jobs;
    const u64 *seg0;
    u64 njobs;
    u8 *out;
    struct State { u64 a, b, obase; };

    __device__ __forceinline__ bool load(const VIndex &V, const FmAnchors &A, u64 t, FmExWalk *w, State *st) const {
        u64 lo = 0, hi = njobs;                                // last job with seg0 <= t
        while (hi - lo > 1) {
            const u64 mid = (lo + hi) >> 1;
            if (seg0[mid] <= t) lo = mid; else hi = mid;
        }
        const FmExJob J = jobs[lo];
        const u64 k = J.klo + (t - seg0[lo]);
        if (k + 1 >= A.na) return false;
        u64 lp, lr;
        fm_anchor(A, V, k, &lp, &lr);
        fm_anchor(A, V, k + 1, &w->p, &w->row);
        w->check = lp >= J.a;
        w->stop = w->check ? lp : J.a;
        w->want_row = lr;
        st->a = J.a; st->b = J.b; st->obase = J.out;
        return w->p > w->stop && w->p < V.n && w->row < V.n && J.b <= V.n && lp < J.b;
    }
    __device__ __forceinline__ bool emit(const FmExWalk &, State *st, u64 pos, u32 sym, u64 *) const {
        if (pos >= st->b) return true;
        if (sym > 3) return false;                             // a separator inside a record: not this index's samples
        out[st->obase + (pos - st->a)] = (u8)(0x54474341u >> (8 * sym));
        return true;
    }
};

// per job: the last anchor at or before a (klo) and the number of anchor gaps up to the first anchor at or after b.
// Anchor 0 is position 0 and the last anchor is n - 1 >= b, so both exist.
__global__ __launch_bounds__(256) void k_fm_extract_plan(VIndex V, FmAnchors A, FmExJob *__restrict__ jobs, u64 njobs,
                                                         u64 *__restrict__ nseg) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    const u64 a = jobs[j].a, b = jobs[j].b;
    if (b <= a) { jobs[j].klo = 0; nseg[j] = 0; return; }
    u64 lo = 0, hi = A.na;                                     // last anchor with position <= a
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        u64 p, r;
        fm_anchor(A, V, mid, &p, &r);
        if (p <= a) lo = mid; else hi = mid;
    }
    const u64 klo = lo;
    hi = A.na - 1;                                             // first anchor with position >= b, above klo
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        u64 p, r;
        fm_anchor(A, V, mid, &p, &r);
        if (p >= b) hi = mid; else lo = mid;
    }
    jobs[j].klo = klo;
    nseg[j] = hi - klo;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------

template <class E>
__global__ __launch_bounds__(256) void k_fm_extract_walk(VIndex V, FmAnchors A, E em, u64 nitems, u32 chunk,
                                                         u64 *__restrict__ ctr) {
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    u64 next = wave * chunk;                                   // wave-uniform: the next item of this wave's run
    if (next >= nitems) return;
    const u64 end = next + chunk < nitems ? next + chunk : nitems;
    FmExWalk w{};
    typename E::State st{};
    bool have = false;
    u64 steps = 0, iters = 0;
    u32 chain = 0, bad = 0;
    for (;;) {
        const u64 idle = __ballot(!have);
        if (idle && next < end) {                              // idle lanes take the next items, in lane order
            const u64 t = next + (u64)__popcll(idle & lanemask_lt());
            if (!have && t < end) {
                if (em.load(V, A, t, &w, &st)) have = true; else bad++;
            }
            next += (u64)__popcll(idle);
        }
        if (!__ballot(have)) {
            if (next >= end) break;
            continue;
        }
        iters++;
        if (have) {
            u32 sym;
            const u64 nr = v_lf(V, w.row, &sym);
            w.p--; steps++;
            bool ok = em.emit(w, &st, w.p, sym, ctr);
            if (nr >= V.n) ok = false;
            w.row = nr;
            if (!ok) { bad++; have = false; }
            else if (w.p == w.stop) {
                if (w.check && w.row != w.want_row) chain++;
                have = false;
            }
        }
    }
    u64 x[3] = {steps, chain, bad};
#pragma unroll
    for (int q = 0; q < 3; q++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x[q] += __shfl_xor(x[q], d, 64);
    }
    if (lane_id() == 0) {
        atomicAdd(&ctr[FM_EX_W_STEPS], x[0]);
        atomicAdd(&ctr[FM_EX_W_WAVE], iters * 64);
        if (x[1]) atomicAdd(&ctr[FM_EX_W_CHAIN], x[1]);
        if (x[2]) atomicAdd(&ctr[FM_EX_W_BAD], x[2]);
    }
}
