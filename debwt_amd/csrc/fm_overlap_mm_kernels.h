// fm_overlap_mm_kernels.h -- suffix-prefix overlaps with up to K mismatches (substitutions): the level-by-level walk of
// k_fm_search joined with the separator-row probe of k_fm_overlap_walk.  A level-L item is (pattern, strand, depth, lo, hi):
// [lo, hi) are the rows of a string W of d = m - depth characters at Hamming distance exactly L from the query's last d
// characters.  A child's letter always differs from the query's, so distinct items are distinct strings, a record prefix
// of d bases equals at most one of them, and every (record, length) is found by exactly one item, whose level is its
// mismatch count: nothing is deduplicated.
//   k_fm_overlap_mm         one lane per item of one level: children into the next level's buffer, one run (pattern, first
//                           srows entry, entries, d | level << 16 | strand << 24) per state that holds record starts
// The host orders the runs and k_fm_overlap_expand (fm_overlap_kernels.h) writes their hits, mismatches in flags >> 8.
// Single TU: included by debwt_hip.hip only, after fm_overlap_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"
#include "fm_search_kernels.h"
#include "fm_mem_kernels.h"
#include "fm_overlap_kernels.h"

// The probe of one state: when d bases are enough and `level` mismatches in d columns are within the rate, the entries
// of srows inside [lo, hi) by the two searches of k_fm_overlap_walk; a run when there are any.  Every lane that steps
// calls it (the append is a wave operation over the calling lanes).
__device__ __forceinline__ void fm_ovl_mm_probe(const VIndex &V, u64 lo, u64 hi, u32 pat, u32 d, u32 level, u32 strand,
                                                u32 min_overlap, u32 permille, uint4 *__restrict__ runs, u64 run_cap,
                                                u64 *__restrict__ ctr) {
    u64 a = 0, b = 0;
    if (lo < hi && d >= min_overlap && (!permille || 1000u * level <= permille * d)) {
        a = lower_bound_dev<u64>(V.srows, 0, V.nsep, lo);
        const u64 span = hi - lo, top = V.nsep - a < span ? V.nsep : a + span;   // srows holds distinct rows
        b = lower_bound_dev<u64>(V.srows, a, top, hi);
    }
    const u64 slot = fm_wave_append(&ctr[1], b > a ? 1u : 0u);
    if (b > a && slot < run_cap) runs[slot] = make_uint4(pat, (u32)a, (u32)(b - a), d | (level << 16) | (strand << 24));
}

// One level.  items_in NULL: level 0, item g = i0 + t is pattern g % np on strand g / np, depth m, interval [0, n).  Else
// item i0 + t of items_in (k_fm_search's layout).  Children (level + 1) go to items_out (capacity out_cap), runs to runs
// (capacity run_cap); both counters count what was asked for, also past the capacity.  permille 0: no rate limit.
// ctr: [0] children asked, [1] runs asked, [2] rank steps, [3] rank lines read, [4] wave steps.
__global__ __launch_bounds__(256) void k_fm_overlap_mm(VIndex V, const u8 *__restrict__ chars, const u64 *__restrict__ offsets,
                                                       u64 base, u64 np, const u64 *__restrict__ items_in, u64 i0, u64 count,
                                                       u32 level, u32 kmax, u32 min_overlap, u32 permille,
                                                       u64 *__restrict__ items_out, u64 out_cap, uint4 *__restrict__ runs,
                                                       u64 run_cap, u64 *__restrict__ ctr) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 steps = 0, reads = 0;
    if (t < count) {                                           // no early return: the wave reductions below need all lanes
        u32 pat, depth, strand;
        u64 lo, hi;
        if (!items_in) {
            const u64 g = i0 + t;
            strand = g >= np ? 1u : 0u;
            pat = (u32)(strand ? g - np : g);
            depth = (u32)(offsets[pat + 1] - offsets[pat]);
            lo = 0; hi = depth ? V.n : 0;
        } else {
            const u64 *it = items_in + 3 * (i0 + t);
            lo = it[0]; hi = it[1];
            const u64 meta = it[2];
            pat = (u32)meta; depth = (u32)(meta >> 32) & 0xFFFFu; strand = (u32)(meta >> 56) & 1u;
        }
        const u64 a = offsets[pat] - base;
        const u32 m = (u32)(offsets[pat + 1] - offsets[pat]);
        // a child spends level + 1 mismatches; its overlaps are at most m long, so past the rate at m it has none
        const bool spawn = level < kmax && (!permille || 1000u * (level + 1) <= permille * m);
        // the state an item of level >= 1 arrives with is the overlap whose leftmost column is the mismatch
        if (items_in) fm_ovl_mm_probe(V, lo, hi, pat, m - depth, level, strand, min_overlap, permille, runs, run_cap, ctr);
        bool alive = lo < hi;
        for (u32 k = depth; alive && k > 0; k--) {
            u32 c = fm_code(chars[strand ? a + m - k : a + k - 1]);
            if (strand && c < 4) c = 3 - c;
            u64 ol[4], oh[4];
            reads += fm_occ4(V, lo, hi, ol, oh);
            steps++;
            u32 nc = 0;
            if (spawn) {
#pragma unroll
                for (u32 b = 0; b < 4; b++) nc += (b != c && oh[b] > ol[b]) ? 1u : 0u;
            }
            u64 slot = fm_wave_append(&ctr[0], nc);
            if (nc) {
                const u64 meta = fm_item_meta(pat, k - 1, level + 1, strand);
#pragma unroll
                for (u32 b = 0; b < 4; b++)
                    if (b != c && oh[b] > ol[b]) {
                        if (slot < out_cap) {
                            u64 *o = items_out + 3 * slot;
                            o[0] = V.C[b] + ol[b]; o[1] = V.C[b] + oh[b]; o[2] = meta;
                        }
                        slot++;
                    }
            }
            if (c > 3) break;                                  // no exact continuation at a non-ACGT character
            const u64 cc = c == 0 ? V.C[0] : c == 1 ? V.C[1] : c == 2 ? V.C[2] : V.C[3];
            const u64 nl = c == 0 ? ol[0] : c == 1 ? ol[1] : c == 2 ? ol[2] : ol[3];
            const u64 nh = c == 0 ? oh[0] : c == 1 ? oh[1] : c == 2 ? oh[2] : oh[3];
            lo = cc + nl; hi = cc + nh;
            alive = lo < hi;
            fm_ovl_mm_probe(V, lo, hi, pat, m - (k - 1), level, strand, min_overlap, permille, runs, run_cap, ctr);
        }
    }
    const u64 wmax = fm_wave_max(steps), ws = fm_wave_sum(steps), wr = fm_wave_sum(reads);
    if (lane_id() == 0 && wmax) {
        atomicAdd((unsigned long long *)&ctr[2], (unsigned long long)ws);
        atomicAdd((unsigned long long *)&ctr[3], (unsigned long long)wr);
        atomicAdd((unsigned long long *)&ctr[4], (unsigned long long)(64 * wmax));
    }
}
