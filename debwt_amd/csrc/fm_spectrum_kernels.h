// fm_spectrum_kernels.h -- the k-mer spectrum of the indexed collection (Definition 9 of include/debwt_hip.h) by direct
// enumeration.  A frontier entry is (lo, hi, code): the non-empty row interval of one string of the current depth and
// its code.  The walk starts from the non-empty entries of the prefix table (depth q) or from [0, n) (depth 0) and one
// expansion per level prepends A, C, G, T with a single fm_occ4: every distinct k-mer is met once, and separator and end
// rows drop out because they belong to none of the four children.  At depth k a leaf kernel takes the multiplicity
// (both strands: one look-up of the reverse complement, walked from its code), and counts it into the histogram or
// appends it to the list.  A frontier is three arrays of `cap` u64 (lo, hi, code); its entries are in no fixed order
// and no result depends on it.  The number of entries of depth d is read from cur[d] on the device, so the levels of a
// chunk are launched back to back over the chunk's bound without a host round trip.
// Single TU: included by debwt_hip.hip only, after fm_kmer_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"
#include "fm_search_kernels.h"
#include "fm_mem_kernels.h"
#include "fm_kmer_kernels.h"

#define FM_SPEC_MAX_K 32u
#define FM_SPEC_MAX_BINS 4096u
#define FM_SPEC_GRANULE 1024u       // table entries per partial sum of k_fm_spectrum_sizes

// counters of the spectrum kernels (u64 each); FM_SP_STEPS: the rank steps of the look-ups (those of the expansions are
// the intervals per depth); FM_SP_LEVEL + d: the intervals of depth d; FM_SP_CUR + d: the frontier cursor of depth d of the
// running chunk (cleared per chunk)
enum { FM_SP_LOOKUPS = 0, FM_SP_STEPS, FM_SP_READS, FM_SP_WSTEPS, FM_SP_OVER, FM_SP_LIST, FM_SP_CLIPPED, FM_SP_LEVEL = 16,
       FM_SP_CUR = FM_SP_LEVEL + FM_SPEC_MAX_K + 1, FM_SP_NCTR = FM_SP_CUR + FM_SPEC_MAX_K + 2 };

__host__ __device__ __forceinline__ u64 fm_spec_mask(u32 k) { return k >= 32 ? ~0ull : (1ull << (2 * k)) - 1; }

// code of the reverse complement of the k-mer of this code: complement every digit, reverse the digits
__host__ __device__ __forceinline__ u64 fm_spec_revcomp(u64 code, u32 k) {
    u64 x = ~code;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    x = (x >> 32) | (x << 32);
    return x >> (64 - 2 * k);
}

// Slots for cnt (0..4) entries per lane of a 256-lane workgroup: the prefix inside the wave from three ballots, the
// waves' totals through LDS, and one returning atomic per workgroup on the cursor.  The rank lines the lanes read
// (0..2 each) ride along in the same LDS words and reach rctr (may be null) with one atomic per workgroup: one atomic per
// wave on a counter that every wave of the grid shares was what the first form of the expansion spent its time on.
// Every lane of the workgroup calls it.
__device__ __forceinline__ u64 fm_spec_slots(u64 *cursor, u32 cnt, u64 *rctr, u32 reads) {
    __shared__ u32 wtot[4];
    __shared__ u64 wbase;
    const u64 b0 = __ballot(cnt & 1u), b1 = __ballot(cnt & 2u), b2 = __ballot(cnt & 4u);
    const u64 below = lanemask_lt();
    const u32 pre = (u32)__popcll(b0 & below) + 2u * (u32)__popcll(b1 & below) + 4u * (u32)__popcll(b2 & below);
    const u32 tot = (u32)__popcll(b0) + 2u * (u32)__popcll(b1) + 4u * (u32)__popcll(b2);
    const u32 wr = (u32)__popcll(__ballot(reads & 1u)) + 2u * (u32)__popcll(__ballot(reads & 2u));
    const u32 w = threadIdx.x >> 6;
    if (lane_id() == 0) wtot[w] = tot | (wr << 16);              // tot <= 256, wr <= 128
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 sum = wtot[0] + wtot[1] + wtot[2] + wtot[3], all = sum & 0xFFFFu, r = sum >> 16;
        wbase = all ? atomicAdd((unsigned long long *)cursor, (unsigned long long)all) : 0ull;
        if (rctr && r) atomicAdd((unsigned long long *)rctr, (unsigned long long)r);
    }
    __syncthreads();
    u32 before = 0;
#pragma unroll
    for (u32 v = 0; v < 3; v++) before += v < w ? (wtot[v] & 0xFFFFu) : 0u;
    return wbase + before + pre;
}

// Sizes of the table in granules of FM_SPEC_GRANULE entries: gsum[2g] = sum of hi - lo, gsum[2g + 1] = non-empty
// entries.  One workgroup of 256 lanes per granule, four entries per lane.
__global__ __launch_bounds__(256) void k_fm_spectrum_sizes(const u64 *__restrict__ table, u64 entries, u64 *__restrict__ gsum) {
    __shared__ u64 part[8];
    const u64 g0 = (u64)blockIdx.x * FM_SPEC_GRANULE;
    u64 s = 0, c = 0;
#pragma unroll
    for (u32 j = 0; j < FM_SPEC_GRANULE / 256; j++) {
        const u64 i = g0 + j * 256 + threadIdx.x;
        if (i < entries) {
            const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(table)[i];
            if (e.y > e.x) { s += e.y - e.x; c++; }
        }
    }
    s = fm_wave_sum(s); c = fm_wave_sum(c);
    if (lane_id() == 0) { part[2 * (threadIdx.x >> 6)] = s; part[2 * (threadIdx.x >> 6) + 1] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        gsum[2 * (u64)blockIdx.x] = part[0] + part[2] + part[4] + part[6];
        gsum[2 * (u64)blockIdx.x + 1] = part[1] + part[3] + part[5] + part[7];
    }
}

// The start frontier of a chunk: the non-empty table entries [i0, i1) with their index as the code (depth q), or, without
// a table, the single entry [0, n) (depth 0).  ctr[FM_SP_CUR + depth] is the frontier's cursor.
__global__ __launch_bounds__(256) void k_fm_spectrum_start(VIndex V, const u64 *__restrict__ table, u64 i0, u64 i1, u32 depth,
                                                           u64 *__restrict__ front, u64 cap, u64 *__restrict__ ctr) {
    const u64 i = i0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 lo = 0, hi = 0;
    if (!table) { if (i == 0) hi = V.n; }
    else if (i < i1) { const ulonglong2 e = reinterpret_cast<const ulonglong2 *>(table)[i]; lo = e.x; hi = e.y; }
    const bool live = hi > lo;
    const u64 slot = fm_spec_slots(&ctr[FM_SP_CUR + depth], live ? 1u : 0u, nullptr, 0u);
    if (live) {
        if (slot < cap) { front[slot] = lo; front[cap + slot] = hi; front[2 * cap + slot] = table ? i : 0ull; }
        else atomicAdd((unsigned long long *)&ctr[FM_SP_CLIPPED], 1ull);
    }
}

// One level: lane t takes entry t of the frontier of this depth (their number is ctr[FM_SP_CUR + depth]), reads its four
// extensions with one fm_occ4 and writes the non-empty ones, the character prepended to the code, to the frontier of
// depth + 1.  No early return: the scan needs all lanes.  The intervals of this depth are the cursor's value, so one lane
// of the grid adds them (and the wave steps, 64 per wave with an entry) to the counters.
__global__ __launch_bounds__(256) void k_fm_spectrum_expand(VIndex V, const u64 *__restrict__ in, u64 *__restrict__ out, u64 cap,
                                                            u32 depth, u64 *__restrict__ ctr) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 count = ctr[FM_SP_CUR + depth] < cap ? ctr[FM_SP_CUR + depth] : cap;
    const bool live = t < count;
    u64 lo = 0, hi = 0, code = 0, ol[4] = {0, 0, 0, 0}, oh[4] = {0, 0, 0, 0};
    u32 reads = 0;
    if (live) {
        lo = in[t]; hi = in[cap + t]; code = in[2 * cap + t];
        reads = fm_occ4(V, lo, hi, ol, oh);
    }
    u32 nc = 0;
#pragma unroll
    for (u32 c = 0; c < 4; c++) nc += oh[c] > ol[c] ? 1u : 0u;
    u64 slot = fm_spec_slots(&ctr[FM_SP_CUR + depth + 1], nc, &ctr[FM_SP_READS], reads);
#pragma unroll
    for (u32 c = 0; c < 4; c++)
        if (oh[c] > ol[c]) {
            if (slot < cap) {
                out[slot] = V.C[c] + ol[c]; out[cap + slot] = V.C[c] + oh[c];
                out[2 * cap + slot] = code | ((u64)c << (2 * depth));
            } else atomicAdd((unsigned long long *)&ctr[FM_SP_CLIPPED], 1ull);      // never, by the chunk's bound
            slot++;
        }
    if (t == 0 && count) {
        atomicAdd((unsigned long long *)&ctr[FM_SP_LEVEL + depth], (unsigned long long)count);
        atomicAdd((unsigned long long *)&ctr[FM_SP_WSTEPS], (unsigned long long)(64 * ((count + 63) / 64)));
    }
}

// occ of the k-mer of this code: from the table entry of its last q characters when k >= q > 0, else from [0, n); one
// fm_occ2 per remaining character while the interval is not empty (fm_kmer_occ, from the code instead of from bytes)
__device__ __forceinline__ u64 fm_spec_occ(const VIndex &V, const u64 *__restrict__ table, u32 q, u64 code, u32 k, u64 &steps,
                                           u64 &reads) {
    u64 lo = 0, hi = V.n;
    u32 x = k;
    if (q) {
        const u64 idx = code & fm_spec_mask(q);
        lo = table[2 * idx]; hi = table[2 * idx + 1];
        x = k - q;
    }
    while (x > 0 && lo < hi) {
        const u32 c = (u32)(code >> (2 * (k - x))) & 3u;       // character x - 1 of the k-mer
        fm_mem_step(V, c, lo, hi, &lo, &hi, steps, reads);
        x--;
    }
    return hi > lo ? hi - lo : 0;
}

// The leaves (depth k).  Forward (both == 0): every leaf W is a member with mult = hi - lo.  Both strands: the leaf
// looks up occ revcomp W and emits the canonical code when W < revcomp W (mult = the sum), W == revcomp W (mult =
// 2 occ) or W > revcomp W with occ revcomp W == 0 (the reverse complement has no leaf of its own).
// hist != null: the histogram of nbins bins in LDS (dynamic, nbins u32), flushed with one u64 atomic per non-zero bin;
// overflow_total from wave reductions (distinct and total follow from the bins and it).  codes != null or hist == null: the members with
// min_mult <= clamped mult <= max_mult are counted in ctr[FM_SP_LIST] and, when codes is there, appended to codes / mults
// (capacity list_cap) from slot list_base on.
__global__ __launch_bounds__(256) void k_fm_spectrum_leaves(VIndex V, const u64 *__restrict__ table, u32 q,
                                                            const u64 *__restrict__ in, u64 cap, u32 k, u32 both, u32 nbins,
                                                            u64 *__restrict__ hist, u32 min_mult, u32 max_mult,
                                                            u64 *__restrict__ codes, u32 *__restrict__ mults, u64 list_cap,
                                                            u64 *__restrict__ ctr) {
    extern __shared__ u32 lhist[];
    if (hist) {
        for (u32 b = threadIdx.x; b < nbins; b += blockDim.x) lhist[b] = 0;
        __syncthreads();
    }
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 count = ctr[FM_SP_CUR + k] < cap ? ctr[FM_SP_CUR + k] : cap;
    const bool live = t < count;
    u64 steps = 0, reads = 0, mult = 0, code = 0;
    bool member = false, looked = false;
    if (live) {
        const u64 lo = in[t], hi = in[cap + t];
        code = in[2 * cap + t];
        mult = hi - lo;
        member = true;
        if (both) {
            const u64 rc = fm_spec_revcomp(code, k);
            if (rc == code) mult *= 2;
            else {
                const u64 orc = fm_spec_occ(V, table, q, rc, k, steps, reads);
                looked = true;
                if (code < rc) mult += orc;
                else { member = orc == 0; code = rc; }
            }
        }
    }
    if (hist) {
        const u64 bin = mult < nbins - 1 ? mult : nbins - 1;
        if (member) atomicAdd(&lhist[bin], 1u);
        // distinct and the total below the last bin follow from the bins on the host; the last bin's total does not
        const u64 wo = fm_wave_sum(member && mult >= nbins - 1 ? mult : 0ull);
        if (lane_id() == 0 && wo) atomicAdd((unsigned long long *)&ctr[FM_SP_OVER], (unsigned long long)wo);
        __syncthreads();
        for (u32 b = threadIdx.x; b < nbins; b += blockDim.x)
            if (lhist[b]) atomicAdd((unsigned long long *)&hist[b], (unsigned long long)lhist[b]);
    } else {
        const u32 m = fm_kmer_clamp(mult);
        const bool pick = member && m >= min_mult && m <= max_mult;
        const u64 slot = fm_wave_append(&ctr[FM_SP_LIST], pick ? 1u : 0u);
        if (pick && codes && slot < list_cap) { codes[slot] = code; mults[slot] = m; }
    }
    if (t == 0 && count) atomicAdd((unsigned long long *)&ctr[FM_SP_LEVEL + k], (unsigned long long)count);
    if (both) {                                                // wave-uniform: the look-ups' counters, per wave
        const u64 wk = (u64)__popcll(__ballot(looked));
        const u64 wmax = fm_wave_max(steps), ws = fm_wave_sum(steps), wr = fm_wave_sum(reads);
        if (lane_id() == 0 && wk) {
            atomicAdd((unsigned long long *)&ctr[FM_SP_LOOKUPS], (unsigned long long)wk);
            atomicAdd((unsigned long long *)&ctr[FM_SP_STEPS], (unsigned long long)ws);
            atomicAdd((unsigned long long *)&ctr[FM_SP_READS], (unsigned long long)wr);
            atomicAdd((unsigned long long *)&ctr[FM_SP_WSTEPS], (unsigned long long)(64 * wmax));
        }
    }
}
