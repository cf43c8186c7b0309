// fm_record_kernels.h -- distinct records per LCP interval from the kept record array (Definition 12 of debwt_hip.h).
//
// Keys.  One lane per row writes da[r] << rb | r, rb the bits of n - 1.  The stable passes of radix_sort_bits over the bits
// [rb, rb + db), db the bits of nrec - 1, put the rows of one record behind one another in row order: neighbours of the
// result with equal da are the pairs (prev[r], r).
//
// Pairs.  One lane per sorted position k >= 1 whose neighbour k - 1 holds the same record finds the leftmost argmin of
// lcp[p + 1 .. r] on the min/max hierarchy of fm_repeat_kernels.h (FmRepTree, built by k_fm_rep_level; only min is read).
// The ascent takes the inclusive range [lo, hi] of a level, reads the entries of lo's node from lo on where lo is not the
// node's first (at most F - 1), the entries of hi's node up to hi where hi is not its last (at most F - 1), and goes on
// with the nodes between them one level up; a range inside one node is read whole (at most F) and ends the ascent.  The
// candidates are disjoint stretches of level 0, so the smallest value with the lowest first row is the leftmost minimum.
// The descent then reads the children of the candidate up to the first that holds the value, at most F per level.  At
// most 3 F reads per level, never a number that grows with r - p.  The lane ends in an integer atomicAdd into dup[m]:
// integer sums do not depend on the order in which the lanes arrive, so dup is the same in every run.
// dup is u32 for n < 2^32 (no value exceeds n - 1) and u64 above.
//
// Scan.  P[r] = dup[0] + .. + dup[r] as plain u64, the kept array: tile sums of 256 rows, k_fm_anc_scan (the rank of the
// extract section) over the tile sums, then the scan inside the tiles.
//
// Gather.  One lane per range: records(lo, hi) = (hi - lo) - (P[hi - 1] - P[lo]), 0 for an empty range.
//
// Single TU: included by debwt_hip.hip only, after fm_repeat_kernels.h.
#pragma once
#include "common.h"
#include "fm_repeat_kernels.h"

#define FM_REC_TILE 256                 // rows per workgroup of the scan

// counters of a build (u64 each)
#define FM_REC_C_PAIRS 0                // rows that have a prev
#define FM_REC_C_STEPS 1                // entries read by the range minimum, every level
#define FM_REC_C_WAVE 2                 // 64 x the reads of the longest lane of every wave and tile
#define FM_REC_C_LOST 3                 // pairs whose descent found no child with the minimum (never)
#define FM_REC_NCTR 8

__global__ __launch_bounds__(256) void k_fm_rec_keys(const u32 *__restrict__ da, u64 n, u32 rb, u64 *__restrict__ keys) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (u64)gridDim.x * blockDim.x)
        keys[r] = ((u64)da[r] << rb) | r;
}

__device__ __forceinline__ u32 fm_rec_min_at(const FmRepTree &T, const u64 *soff, u32 t, u64 pos) {
    return t == 0 ? T.lcp[pos] : T.node[soff[t] + pos].x;
}

// the smallest row of [lo, hi] that holds min(lcp[lo .. hi]); lo <= hi < n.  ~0 when the descent fails (never).
__device__ __forceinline__ u64 fm_rec_argmin(const FmRepTree &T, const u64 *sn, const u64 *soff, u64 lo, u64 hi, u64 *steps) {
    const u64 fm = (1ull << T.sh) - 1;
    u32 bv = 0xFFFFFFFFu, bt = 0;
    u64 bpos = 0, bstart = ~0ull;
    u32 t = 0;
#define FM_REC_TAKE(pos_)                                                                       \
    do {                                                                                        \
        ++*steps;                                                                               \
        const u32 v_ = fm_rec_min_at(T, soff, t, (pos_));                                       \
        const u64 s_ = (pos_) << (T.sh * t);                   /* its first row */              \
        if (v_ < bv || (v_ == bv && s_ < bstart)) { bv = v_; bt = t; bpos = (pos_); bstart = s_; } \
    } while (0)
    for (;;) {
        u64 nlo = lo >> T.sh, nhi = hi >> T.sh;
        if (t == T.levels || nlo == nhi) {
            for (u64 pos = lo; pos <= hi; pos++) FM_REC_TAKE(pos);
            break;
        }
        if (lo & fm) {                                         // lo's node begins left of the range
            const u64 end = (nlo + 1) << T.sh;
            for (u64 pos = lo; pos < end; pos++) FM_REC_TAKE(pos);
            nlo++;
        }
        if ((hi & fm) != fm && hi + 1 < sn[t]) {               // hi's node ends right of the range
            for (u64 pos = nhi << T.sh; pos <= hi; pos++) FM_REC_TAKE(pos);
            nhi--;
        }
        if (nlo > nhi) break;
        lo = nlo; hi = nhi; t++;
    }
#undef FM_REC_TAKE
    while (bt > 0) {                                           // the first child that holds the minimum
        bt--;
        u64 pos = bpos << T.sh;
        const u64 end = pos + fm + 1 < sn[bt] ? pos + fm + 1 : sn[bt];
        for (;;) {
            if (pos >= end) return ~0ull;                      // never: the node above said so
            ++*steps;
            if (fm_rec_min_at(T, soff, bt, pos) == bv) break;
            pos++;
        }
        bpos = pos;
    }
    return bpos;
}

// One lane per sorted position, a tile of 256 per workgroup and step of its stride.  DT: u32 or u64, the type of dup.
template <typename DT>
__global__ __launch_bounds__(256) void k_fm_rec_pairs(FmRepTree T, const u64 *__restrict__ keys, u32 rb, DT *__restrict__ dup,
                                                      u64 *__restrict__ ctr) {
    __shared__ u64 sn[FM_REP_MAXLEV + 1], soff[FM_REP_MAXLEV + 1];
    for (u32 k = threadIdx.x; k <= T.levels; k += blockDim.x) { sn[k] = T.lev[2 * k]; soff[k] = T.lev[2 * k + 1]; }
    __syncthreads();
    const u64 n = sn[0], rmask = rb >= 64 ? ~0ull : (1ull << rb) - 1;
    u64 pairs = 0, steps = 0, wave = 0, lost = 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n; base += (u64)gridDim.x * blockDim.x) {
        const u64 k = base + threadIdx.x;
        u64 mine = 0;
        if (k >= 1 && k < n) {
            const u64 a = keys[k - 1], b = keys[k];
            const u64 p = a & rmask, r = b & rmask;
            if (rb < 64 && (a >> rb) == (b >> rb) && p < r && r < n) {     // p < r < n: the sort is stable, keys hold rows
                pairs++;
                const u64 m = fm_rec_argmin(T, sn, soff, p + 1, r, &mine);
                // an integer sum: the same whatever order the lanes arrive in
                if (m < n) atomicAdd(&dup[m], (DT)1);
                else lost++;
            }
        }
        steps += mine;
        u64 wmax = mine;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(wmax, d, 64); wmax = o > wmax ? o : wmax; }
        wave += wmax;                                          // the same in every lane
    }
    u64 v[3] = {pairs, steps, lost};
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += __shfl_xor(v[k], d, 64);
    }
    if (lane_id() == 0) {
        if (v[0]) atomicAdd(&ctr[FM_REC_C_PAIRS], v[0]);
        if (v[1]) atomicAdd(&ctr[FM_REC_C_STEPS], v[1]);
        if (v[2]) atomicAdd(&ctr[FM_REC_C_LOST], v[2]);
        if (wave) atomicAdd(&ctr[FM_REC_C_WAVE], wave * 64);
    }
}

// inclusive scan of one value per lane over a 256-thread block; *total = block sum.  smem: DEBWT_WAVES u64.
__device__ __forceinline__ u64 fm_rec_block_scan(u64 v, u64 *smem, u64 *total) {
    u64 incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(incl, d, 64);
        if ((int)lane_id() >= d) incl += o;
    }
    const u32 w = threadIdx.x >> 6;
    if (lane_id() == 63) smem[w] = incl;
    __syncthreads();
    u64 base = 0, sum = 0;
#pragma unroll
    for (u32 i = 0; i < DEBWT_WAVES; i++) {
        const u64 s = smem[i];
        if (i < w) base += s;
        sum += s;
    }
    *total = sum;
    return base + incl;
}

// scan, pass 1: the sum of every tile of FM_REC_TILE rows
template <typename DT>
__global__ __launch_bounds__(FM_REC_TILE) void k_fm_rec_tile_sums(const DT *__restrict__ dup, u64 n, u64 *__restrict__ tsum) {
    __shared__ u64 smem[DEBWT_WAVES];
    const u64 r = (u64)blockIdx.x * FM_REC_TILE + threadIdx.x;
    u64 total;
    (void)fm_rec_block_scan(r < n ? (u64)dup[r] : 0ull, smem, &total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// scan, pass 3: toff holds the exclusive scan of the tile sums (k_fm_anc_scan)
template <typename DT>
__global__ __launch_bounds__(FM_REC_TILE) void k_fm_rec_scan(const DT *__restrict__ dup, u64 n, const u64 *__restrict__ toff,
                                                             u64 *__restrict__ P) {
    __shared__ u64 smem[DEBWT_WAVES];
    const u64 r = (u64)blockIdx.x * FM_REC_TILE + threadIdx.x;
    u64 total;
    const u64 incl = fm_rec_block_scan(r < n ? (u64)dup[r] : 0ull, smem, &total);
    if (r < n) P[r] = toff[blockIdx.x] + incl;
}

// One lane per range [lo, hi), the host checked lo <= hi <= n
__global__ __launch_bounds__(256) void k_fm_rec_gather(const u64 *__restrict__ P, u64 n, const u64 *__restrict__ ranges, u64 nranges,
                                                       u64 *__restrict__ out) {
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < nranges; k += (u64)gridDim.x * blockDim.x) {
        const u64 lo = ranges[2 * k], hi = ranges[2 * k + 1];
        out[k] = lo < hi && hi <= n ? (hi - lo) - (P[hi - 1] - P[lo]) : 0ull;
    }
}
