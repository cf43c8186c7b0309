// fm_mem_kernels.h -- maximal exact matches (MEMs) of patterns against the FM-index, with backward search only.  One
// lane per (pattern, strand) item works from the pattern's right end: it walks left from the current end e with
// fm_occ2 while the interval stays non-empty (s(e), the smallest start that still occurs), emits [s(e), e + 1) when it
// is long enough, then finds the next end that can be a MEM end by a binary search over e' with P[s - 1 .. e'] occurring
// and resumes the walk from that probe's interval.  The host gives every item a slot range of its worst-case MEM count
// (max(0, m - min_len + 1)) and compacts (debwt_fm_mems).
// Single TU: included by debwt_hip.hip only, after fm_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"

__device__ __forceinline__ u64 fm_wave_sum(u64 v) {          // over the 64 lanes of a full wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u32 lo = (u32)__shfl_xor((int)(u32)v, o, 64), hi = (u32)__shfl_xor((int)(u32)(v >> 32), o, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ u64 fm_wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u32 lo = (u32)__shfl_xor((int)(u32)v, o, 64), hi = (u32)__shfl_xor((int)(u32)(v >> 32), o, 64);
        const u64 w = ((u64)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// code of position x (0-based, left to right) of the item's query string: the pattern itself (strand 0) or its reverse
// complement (strand 1), read from the same bytes; 4 for a character outside ACGTacgt
__device__ __forceinline__ u32 fm_mem_code(const u8 *__restrict__ p, u64 m, u32 strand, u64 x) {
    if (!strand) return fm_code(p[x]);
    const u32 c = fm_code(p[m - 1 - x]);
    return c < 4 ? 3u - c : c;
}

// One backward-search step: [lo, hi) of W -> [lo, hi) of cW.  Counts the step and the rank lines fm_occ2 reads.
__device__ __forceinline__ void fm_mem_step(const VIndex &V, u32 c, u64 lo, u64 hi, u64 *nl, u64 *nh, u64 &steps,
                                            u64 &reads) {
    u64 ol, oh;
    fm_occ2(V, c, lo, hi, &ol, &oh);
    steps++;
    reads += lo / VB_ROWS == hi / VB_ROWS ? 1u : 2u;
    const u64 cc = c == 0 ? V.C[0] : c == 1 ? V.C[1] : c == 2 ? V.C[2] : V.C[3];
    *nl = cc + ol; *nh = cc + oh;
}

// MEMs of items [0, nitems): item g is pattern g % np on strand g / np (like level 0 of k_fm_search).  Positions below
// are exclusive ends E = e + 1 and starts S in the item's query string; a MEM [S, E) of strand 1 is written as
// [m - E, m - S) of the pattern as given.  Item g writes its MEMs, in descending E, to slots slot_base[g] .. (at most
// slot_base[g + 1] - slot_base[g] of them): spans (2 u32 each) and ranges (2 u64, [lo, hi) as k_fm_count gives them),
// and their number to counts[g].  ctr: [0] rank steps, [1] rank lines read, [2] wave steps (64 x the longest lane of
// each wave: what the waves issue, so steps / wave steps is the SIMD efficiency).
__global__ __launch_bounds__(256) void k_fm_mems(VIndex V, const u8 *__restrict__ chars, const u64 *__restrict__ offsets,
                                                 u64 base, u64 np, u64 nitems, u32 min_len,
                                                 const u64 *__restrict__ slot_base, u32 *__restrict__ spans,
                                                 u64 *__restrict__ ranges, u32 *__restrict__ counts,
                                                 u64 *__restrict__ ctr) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 steps = 0, reads = 0;
    if (g < nitems) {                                          // no early return: the wave reductions below need all lanes
        const u32 strand = g >= np ? 1u : 0u;
        const u64 j = strand ? g - np : g;
        const u64 m = offsets[j + 1] - offsets[j];
        const u8 *p = chars + (offsets[j] - base);
        const u64 s0 = slot_base[g], cap = slot_base[g + 1] - s0;
        u64 nm = 0;
        // One rank step per turn, from the walk or from a probe of the binary search, so the lanes of a wave share the
        // fm_occ2 call whichever phase each is in.  Walk: [lo, hi) is the interval of Q[S, E).  Probe: [pl, ph) is the
        // interval of Q[k, mid), heading for k = S - 1; good / bad bracket the next end (Q[S - 1, good) occurs, Q[S - 1,
        // bad) does not).
        u64 E = cap ? m : 0, S = E, lo = 0, hi = V.n;          // m < min_len: no MEM, nothing to do
        u64 good = 0, bad = 0, mid = 0, k = 0, pl = 0, ph = 0, glo = 0, ghi = 0;
        bool probe = false;
        while (E > 0) {
            u32 c = 4;
            if (probe) c = fm_mem_code(p, m, strand, k - 1);   // Q[S - 1, E - 1) occurs: all bases
            else if (S > 0) c = fm_mem_code(p, m, strand, S - 1);
            bool ok = false;
            if (c <= 3) {
                u64 nl, nh;
                fm_mem_step(V, c, probe ? pl : lo, probe ? ph : hi, &nl, &nh, steps, reads);
                ok = nl < nh;
                if (ok && probe) { pl = nl; ph = nh; k--; }
                else if (ok) { lo = nl; hi = nh; S--; }
            }
            if (probe) {
                if (ok && k > S - 1) continue;
                if (ok) { good = mid; glo = pl; ghi = ph; } else bad = mid;
                if (bad - good > 1) { mid = good + (bad - good) / 2; k = mid; pl = 0; ph = V.n; continue; }
                probe = false;                                 // next end found: resume from Q[S - 1, good) when probed
                E = good;
                if (ghi > glo) { S--; lo = glo; hi = ghi; } else { S = E; lo = 0; hi = V.n; }
                continue;
            }
            if (ok) continue;
            // the walk stopped: S = s(E - 1)
            if (S < E && E - S >= min_len && nm < cap) {
                const u64 o = s0 + nm;
                spans[2 * o] = (u32)(strand ? m - E : S); spans[2 * o + 1] = (u32)(strand ? m - S : E);
                ranges[2 * o] = lo; ranges[2 * o + 1] = hi;
                nm++;
            }
            if (S == 0) break;
            if (S == E) { E--; S = E; lo = 0; hi = V.n; continue; }          // Q[E - 1] matches nothing
            const u32 cp = fm_mem_code(p, m, strand, S - 1);
            const u64 rows = cp == 0 ? V.C[1] - V.C[0] : cp == 1 ? V.C[2] - V.C[1] : cp == 2 ? V.C[3] - V.C[2] : V.C[4] - V.C[3];
            if (cp > 3 || rows == 0) { E = S - 1; S = E; lo = 0; hi = V.n; continue; }
            // next end: the largest E' in [S, E) with Q[S - 1, E') occurring (E' = S holds, E does not).  Every end
            // between it and E has s = S, so none of them ends a MEM.
            good = S; bad = E; glo = ghi = 0;
            if (bad - good > 1) { probe = true; mid = good + (bad - good) / 2; k = mid; pl = 0; ph = V.n; continue; }
            E = good; S = E; lo = 0; hi = V.n;
        }
        counts[g] = (u32)nm;
    }
    const u64 wmax = fm_wave_max(steps), ws = fm_wave_sum(steps), wr = fm_wave_sum(reads);
    if (lane_id() == 0 && wmax) {
        atomicAdd((unsigned long long *)&ctr[0], (unsigned long long)ws);
        atomicAdd((unsigned long long *)&ctr[1], (unsigned long long)wr);
        atomicAdd((unsigned long long *)&ctr[2], (unsigned long long)(64 * wmax));
    }
}

// Compaction: item g's counts[g] MEMs move from slot_base[g] to out_base[g], ascending by start (strand 0 items were
// written in descending E, so they are reversed; strand 1 items already ascend in the pattern's coordinates).
__global__ __launch_bounds__(256) void k_fm_mems_compact(const u64 *__restrict__ slot_base, const u32 *__restrict__ counts,
                                                         const u64 *__restrict__ out_base, u64 np, u64 nitems,
                                                         const u32 *__restrict__ spans, const u64 *__restrict__ ranges,
                                                         u32 *__restrict__ spans_out, u64 *__restrict__ ranges_out) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nitems) return;
    const u64 a = slot_base[g], o = out_base[g], c = counts[g];
    const bool rev = g < np;
    for (u64 k = 0; k < c; k++) {
        const u64 src = a + (rev ? c - 1 - k : k), dst = o + k;
        spans_out[2 * dst] = spans[2 * src]; spans_out[2 * dst + 1] = spans[2 * src + 1];
        ranges_out[2 * dst] = ranges[2 * src]; ranges_out[2 * dst + 1] = ranges[2 * src + 1];
    }
}
