// fm_overlap_kernels.h -- suffix-prefix overlaps of patterns against the records of the collection.  The rows whose BWT
// symbol is a separator (VIndex.srows) are the rows of the suffixes that start at the first base of a record, so after a
// backward search of the last d bases of a query the records that start with those bases are the entries of srows inside
// [lo, hi): two binary searches, no LF walk.  One backward walk of the query gives every overlap length.
//   k_fm_overlap_walk     one lane per (pattern, strand): the walk; a run (depth, first srows entry, entries) per depth with
//                         at least one record, into the item's slots (max(0, m - min_overlap + 1), host prefix sum)
//   k_fm_overlap_compact  one lane per item: its runs, deepest first, to their final place with their first hit number
//   k_fm_overlap_expand   one lane per hit: its run by binary search, then (record, length, strand, flags)
// Single TU: included by debwt_hip.hip only, after fm_mem_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"
#include "fm_mem_kernels.h"

// one entry of the record table per entry of srows: the record that starts at that row and its length in bases
// (lengths of 2^32 - 1 and above are stored as 2^32 - 1)
struct FmOvlRec { u32 record, length; };

// A run as the walk writes it: x = depth (overlap length), y = first entry of srows, z = entries, w unused.  As the
// compaction writes it: w = strand | 2 when the depth is the whole query; the mismatch call's host adds mismatches << 8.
typedef uint4 FmOvlRun;

// Items [0, nitems): item g is pattern g % np on strand g / np, as in k_fm_mems.  Item g writes its runs in ascending
// depth to slots slot_base[g] .. (slot_base[g + 1] - slot_base[g] of them: one per depth >= min_overlap, so they cannot
// overflow), their number to nruns[g] and the sum of their entries to nhits[g].  ctr as in k_fm_mems: [0] rank steps,
// [1] rank lines read, [2] wave steps.
__global__ __launch_bounds__(256) void k_fm_overlap_walk(VIndex V, const u8 *__restrict__ chars, const u64 *__restrict__ offsets,
                                                         u64 base, u64 np, u64 nitems, u32 min_overlap,
                                                         const u64 *__restrict__ slot_base, FmOvlRun *__restrict__ runs,
                                                         u32 *__restrict__ nruns, u64 *__restrict__ nhits,
                                                         u64 *__restrict__ ctr) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 steps = 0, reads = 0;
    if (g < nitems) {                                          // no early return: the wave reductions below need all lanes
        const u32 strand = g >= np ? 1u : 0u;
        const u64 j = strand ? g - np : g;
        const u64 m = offsets[j + 1] - offsets[j];
        const u8 *p = chars + (offsets[j] - base);
        const u64 s0 = slot_base[g], cap = slot_base[g + 1] - s0;
        u64 lo = 0, hi = V.n, d = 0, nr = 0, nh = 0;
        while (cap && d < m) {                                 // m < min_overlap: no slots, nothing to do
            const u32 c = fm_mem_code(p, m, strand, m - 1 - d);
            if (c > 3) break;
            u64 nl, nu;
            fm_mem_step(V, c, lo, hi, &nl, &nu, steps, reads);
            if (nl >= nu) break;
            lo = nl; hi = nu; d++;
            if (d < min_overlap) continue;
            // srows holds distinct rows, so at most hi - lo of them lie in [lo, hi): the second search is short
            const u64 a = lower_bound_dev<u64>(V.srows, 0, V.nsep, lo);
            const u64 span = hi - lo, top = V.nsep - a < span ? V.nsep : a + span;
            const u64 b = lower_bound_dev<u64>(V.srows, a, top, hi);
            if (b > a && nr < cap) {
                runs[s0 + nr] = make_uint4((u32)d, (u32)a, (u32)(b - a), 0u);
                nr++; nh += b - a;
            }
        }
        nruns[g] = (u32)nr; nhits[g] = nh;
    }
    const u64 wmax = fm_wave_max(steps), ws = fm_wave_sum(steps), wr = fm_wave_sum(reads);
    if (lane_id() == 0 && wmax) {
        atomicAdd((unsigned long long *)&ctr[0], (unsigned long long)ws);
        atomicAdd((unsigned long long *)&ctr[1], (unsigned long long)wr);
        atomicAdd((unsigned long long *)&ctr[2], (unsigned long long)(64 * wmax));
    }
}

// Compaction: item g's nruns[g] runs move from slot_base[g] to run_base[g] in descending depth, and run_out gets the
// number of each run's first hit, counted from hit_base[g] (both bases from the host, in (pattern, strand) order).
__global__ __launch_bounds__(256) void k_fm_overlap_compact(const u64 *__restrict__ offsets, const u64 *__restrict__ slot_base,
                                                            const u32 *__restrict__ nruns, const u64 *__restrict__ run_base,
                                                            const u64 *__restrict__ hit_base, u64 np, u64 nitems,
                                                            const FmOvlRun *__restrict__ runs, FmOvlRun *__restrict__ cruns,
                                                            u64 *__restrict__ run_out) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nitems) return;
    const u32 strand = g >= np ? 1u : 0u;
    const u64 j = strand ? g - np : g;
    const u64 m = offsets[j + 1] - offsets[j];
    const u64 a = slot_base[g], o = run_base[g], c = nruns[g];
    u64 h = hit_base[g];
    for (u64 k = 0; k < c; k++) {
        FmOvlRun r = runs[a + (c - 1 - k)];
        r.w = strand | (r.x == m ? 2u : 0u);
        cruns[o + k] = r;
        run_out[o + k] = h;
        h += r.z;
    }
}

// Expansion, for the exact and the mismatch call alike: one lane per hit g in [g0, g0 + count) of the batch.  Run k covers
// hits [run_out[k], run_out[k + 1]) (the last one to the batch's end); the hit is entry y + (g - run_out[k]) of the
// record table.  A run's w: bit 0 the strand, bit 1 set when the length is the whole query, bits 8..15 the mismatches --
// zero from k_fm_overlap_compact, the level from the host's ordering of k_fm_overlap_mm's runs.  out[t]: record, length,
// strand, flags (1: the record is as long as the overlap, 2: the query is, mismatches << 8), in row order inside one run.
__global__ __launch_bounds__(256) void k_fm_overlap_expand(const FmOvlRun *__restrict__ cruns, const u64 *__restrict__ run_out,
                                                           u64 nruns, const FmOvlRec *__restrict__ table, u64 g0, u64 count,
                                                           uint4 *__restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const u64 g = g0 + t;
    u64 lo = 0, hi = nruns;                                    // last run with run_out[k] <= g
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (run_out[mid] <= g) lo = mid; else hi = mid;
    }
    const FmOvlRun r = cruns[lo];
    const FmOvlRec e = table[(u64)r.y + (g - run_out[lo])];
    out[t] = make_uint4(e.record, r.x, r.w & 1u, (e.length == r.x ? 1u : 0u) | (r.w & 0xFF02u));
}
