// fm_esa_kernels.h -- the classical companions of the BWT (Definition 10 of debwt_hip.h): the full suffix array, the
// LCP array and the record (document) array of the indexed collection.
//
// Suffix array.  A third emitter of k_fm_extract_walk: item t is the gap between anchors t and t + 1, and every step
// stores the position of the row it leaves, so item t writes the rows of positions (lower, upper]; item 0 also writes
// position 0 on the '$' row.  The chain check of the walk stays: when every item arrives on the row of its lower anchor
// the n - 1 steps are one LF cycle and every row was written exactly once.
//
// PLCP.  phi[sa[r]] = sa[r - 1] is scattered, and the text positions are cut into chunks: one lane per chunk walks its
// positions in text order and carries the match length from one to the next, minus one (Kasai), starting from 0 at the
// chunk's first position.  The compare is word-wise, 32 bases per step through text_window; separators are packed as
// 'T', so the same step reads the separator bitmap at both suffixes and stops at the first separator of either.  A
// chunk costs its length in steps plus at most the cap for its restart: n + chunks x cap symbols, whatever the sum of
// the LCP values is.  The reads of a lane are dependent and scattered (phi, then two text windows); the kernel lives
// on lanes in flight, as k_fm_count does.
//
// Row order.  One lane per row gathers lcp[r] = plcp[sa[r]], finds the record of sa[r] by a rank over the separator
// bitmap (da, and d = the bases up to the record's separator), adds +1 at lcp + 1 and -1 at d + 1 to a difference array
// in LDS (clamped to FM_ESA_KMAX + 1) and reduces sum, capped count and maximum per wave.  A second pass finds the first
// row of the maximum.
// Single TU: included by debwt_hip.hip only, after fm_extract_kernels.h.
#pragma once
#include "common.h"
#include "fm_extract_kernels.h"

#define FM_ESA_KMAX 4096u               // longest k of the profile
#define FM_ESA_NDIFF (FM_ESA_KMAX + 2)  // difference array: entries 1 .. KMAX + 1 are used

// counters of a build (u64 each), behind them the difference array
#define FM_ESA_C_SYMBOLS 0              // symbol pairs examined by k_fm_esa_plcp, 32 per word step
#define FM_ESA_C_WAVE 1                 // 64 x the word steps of the longest lane of every wave
#define FM_ESA_C_SUM 2
#define FM_ESA_C_CAPPED 3
#define FM_ESA_C_MAX 4
#define FM_ESA_C_MAXROW 5               // set to ~0 before k_fm_esa_maxrow
#define FM_ESA_C_BADPHI 6               // positions whose phi is no text position (never with a checked walk)
#define FM_ESA_NCTR 8

// Every row the walk leaves gets its position.  emit() runs after the step: w.row is still the row of pos + 1.
struct FmExSa {
    u64 *sa;               // n entries
    struct State {};

    __device__ __forceinline__ bool load(const VIndex &V, const FmAnchors &A, u64 t, FmExWalk *w, State *) const {
        u64 lp, lr;
        fm_anchor(A, V, t, &lp, &lr);
        fm_anchor(A, V, t + 1, &w->p, &w->row);
        w->stop = lp; w->want_row = lr; w->check = true;
        bool ok = w->p > lp && w->p < V.n && w->row < V.n;
        if (t == 0) {                                          // the text begins on the '$' row: no walk leaves it
            if (lp != 0 || lr != V.dollar_row) ok = false;
            else sa[lr] = 0;
        }
        return ok;
    }
    __device__ __forceinline__ bool emit(const FmExWalk &w, State *, u64 pos, u32, u64 *) const {
        sa[w.row] = pos + 1;                                   // w.row < n: checked by load and after every step
        return true;
    }
};

__global__ __launch_bounds__(256) void k_fm_esa_phi(const u64 *__restrict__ sa, u64 n, u64 *__restrict__ phi) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u64 p = sa[r];
    if (p < n) phi[p] = r ? sa[r - 1] : ~0ull;                // row 0 has no row before it
}

// One lane per chunk of `chunk` text positions.  plcp[i] = min(cut common prefix of suffixes i and phi[i], cap).
__global__ __launch_bounds__(256) void k_fm_esa_plcp(const u64 *__restrict__ text, const u64 *__restrict__ sepbits,
                                                     const u64 *__restrict__ phi, u64 n, u64 chunk, u64 nchunks, u64 cap,
                                                     u32 *__restrict__ plcp, u64 *__restrict__ ctr) {
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 words = 0, bad = 0;
    if (c < nchunks) {
        const u64 lo = c * chunk, hi = lo + chunk < n ? lo + chunk : n;
        u64 h = 0;
        for (u64 i = lo; i < hi; i++) {
            const u64 j = phi[i];
            h = h ? h - 1 : 0;
            if (j >= n) { if (j != ~0ull) bad++; h = 0; }
            else {
                // i + h and j + h never pass a separator, and position n - 1 is one: both stay below n
                while (h < cap && i + h < n && j + h < n) {
                    const u64 x = text_window(text, i + h) ^ text_window(text, j + h);
                    const u32 s = (u32)sep_window(sepbits, i + h) | (u32)sep_window(sepbits, j + h);
                    const u32 mis = x ? (u32)__clzll(x) >> 1 : 32u;
                    const u32 stop = s ? (u32)__ffs(s) - 1u : 32u;
                    const u32 m = mis < stop ? mis : stop;
                    words++;
                    h += m;
                    if (m < 32) break;
                }
                if (h > cap) h = cap;
            }
            plcp[i] = (u32)h;
        }
    }
    u64 wmax = words;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        words += __shfl_xor(words, d, 64);
        bad += __shfl_xor(bad, d, 64);
        const u64 o = __shfl_xor(wmax, d, 64);
        wmax = o > wmax ? o : wmax;
    }
    if (lane_id() == 0) {
        if (words) atomicAdd(&ctr[FM_ESA_C_SYMBOLS], words * 32);
        if (wmax) atomicAdd(&ctr[FM_ESA_C_WAVE], wmax * 64);
        if (bad) atomicAdd(&ctr[FM_ESA_C_BADPHI], bad);
    }
}

// The record of sa[r] is the number of separators before it: a rank over the separator bitmap in the layout of the
// anchor rank (k_fm_anc_count, k_fm_anc_scan: wpre per word inside chunks of FM_EX_CHUNK_WORDS words, csum per chunk),
// three reads where a search in the record starts took log2(nrec) dependent ones.  seps: the nrec separator positions,
// ascending.  da may be null.  diff: FM_ESA_NDIFF u64, added to.  Any grid: a workgroup takes at most 2^31 rows, the
// range of its LDS counters.
__global__ __launch_bounds__(256) void k_fm_esa_rows(const u64 *__restrict__ sa, const u32 *__restrict__ plcp,
                                                     const u64 *__restrict__ sepbits, const u32 *__restrict__ wpre,
                                                     const u64 *__restrict__ csum, const u64 *__restrict__ seps, u64 nrec,
                                                     u64 n, u32 cap, u32 count_capped, u32 *__restrict__ lcp,
                                                     u32 *__restrict__ da, u64 *__restrict__ ctr, u64 *__restrict__ diff) {
    __shared__ int sdiff[FM_ESA_NDIFF];
    for (u32 k = threadIdx.x; k < FM_ESA_NDIFF; k += blockDim.x) sdiff[k] = 0;
    __syncthreads();
    u64 sum = 0, capped = 0;
    u32 mx = 0;
    // a workgroup strides over the rows: its LDS array is cleared and flushed once, and every wave adds its sums once
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (u64)gridDim.x * blockDim.x) {
        const u64 p = sa[r];
        u32 l = 0;
        u64 d = 0;
        if (p < n) {
            l = plcp[p];
            const u64 w = p >> 6;
            u64 j = csum[w / FM_EX_CHUNK_WORDS] + wpre[w] + (u64)__popcll(sepbits[w] & ((1ull << (p & 63)) - 1ull));
            if (j >= nrec) j = nrec - 1;                       // never with the bitmap of these separators
            const u64 sp = seps[j];
            d = sp > p ? sp - p : 0;
            if (da) da[r] = (u32)j;
        }
        lcp[r] = l;
        sum += l;
        mx = l > mx ? l : mx;
        capped += count_capped && l == cap ? 1 : 0;
        const u32 up = l < FM_ESA_KMAX ? l + 1 : FM_ESA_KMAX + 1;
        const u32 dn = d < FM_ESA_KMAX ? (u32)d + 1 : FM_ESA_KMAX + 1;
        if (up != dn) {                                        // entry KMAX + 1 is in no prefix sum: not counted
            if (up <= FM_ESA_KMAX) atomicAdd(&sdiff[up], 1);
            if (dn <= FM_ESA_KMAX) atomicAdd(&sdiff[dn], -1);
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        sum += __shfl_xor(sum, s, 64);
        capped += __shfl_xor(capped, s, 64);
        const u32 o = __shfl_xor(mx, s, 64);
        mx = o > mx ? o : mx;
    }
    if (lane_id() == 0) {
        if (sum) atomicAdd(&ctr[FM_ESA_C_SUM], sum);
        if (capped) atomicAdd(&ctr[FM_ESA_C_CAPPED], capped);
        if (mx) atomicMax(&ctr[FM_ESA_C_MAX], (u64)mx);
    }
    __syncthreads();
    for (u32 k = threadIdx.x; k < FM_ESA_NDIFF; k += blockDim.x) {
        const int v = sdiff[k];
        if (v) atomicAdd(&diff[k], (u64)(long long)v);         // two's complement: the sums are taken modulo 2^64
    }
}

// the first row that holds the maximum
__global__ __launch_bounds__(256) void k_fm_esa_maxrow(const u32 *__restrict__ lcp, u64 n, u64 *__restrict__ ctr) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 mx = ctr[FM_ESA_C_MAX];
    u64 row = r < n && lcp[r] == mx ? r : ~0ull;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 o = __shfl_xor(row, s, 64);
        row = o < row ? o : row;
    }
    if (lane_id() == 0 && row != ~0ull) atomicMin(&ctr[FM_ESA_C_MAXROW], row);
}
