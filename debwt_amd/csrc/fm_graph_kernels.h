// fm_graph_kernels.h -- the string graph of the indexed records: states, longest-overlap edges among the kept records,
// their transitive reduction.  The overlap walk, compaction and expansion are those of fm_overlap_kernels.h, launched
// unchanged on records unpacked from the attached text.
//   k_fm_graph_unpack   one lane per base of a batch of records: the 2-bit text as upper-case ACGT for the walk
//   k_fm_graph_state    one lane per record: backward search of the whole record, then duplicate / contained / kept
//   k_fm_graph_pack     one lane per expanded hit of a chunk: (record, length) of a hit between two kept records, or a gap
//   k_fm_graph_longest  one lane per packed hit: keep it when no earlier hit of its source names the same record
//   k_fm_graph_degree   one lane per source: the kept entries of its segment
//   k_fm_graph_scatter  one lane per kept entry: to its place in the compacted list
//   k_fm_graph_reduce   one lane per edge: the keep bit of the transitive reduction (the hot path)
// Single TU: included by debwt_hip.hip only, after fm_overlap_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"
#include "fm_mem_kernels.h"
#include "fm_overlap_kernels.h"

struct FmEdge { u32 record, length; };                 // debwt_fm_edge
constexpr u32 FM_GRAPH_GAP = 0xFFFFFFFFu;              // FmEdge.record of a hit that is no edge

// counters of the graph kernels (u64 each)
enum { FM_GR_BADLEN = 0, FM_GR_LOOKUPS = 1, FM_GR_REDUCIBLE = 2, FM_GR_NCTR = 8 };

// last s in [0, nseg) with seg[s] <= g; seg ascending with seg[0] <= g < seg[nseg]
__device__ __forceinline__ u64 fm_graph_segment(const u64 *__restrict__ seg, u64 nseg, u64 g) {
    u64 lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (seg[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// Bases [0, count) of records [p0, p0 + np): coff[r] = the bases before record r (np + 1 entries from coff + p0 are read),
// so base c of the collection stands at text position c + r.  out[t] is base coff[p0] + t.
__global__ __launch_bounds__(256) void k_fm_graph_unpack(const u64 *__restrict__ text, const u64 *__restrict__ coff, u64 p0, u64 np,
                                                         u64 count, u8 *__restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const u64 c = coff[p0] + t;
    const u64 r = p0 + fm_graph_segment(coff + p0, np, c);
    out[t] = (u8)((0x54474341u >> (8 * text_symbol(text, c + r))) & 0xFFu);      // "ACGT"
}

// State of record i: the rows [lo, hi) of the suffixes that start with S_i are its occurrences; the entries of srows in
// [lo, hi) are the records that start with S_i, and those of its length are its copies, itself included.
// 1: a copy has a smaller number; else 2: it occurs more often than it has copies (inside a longer record); else 0.
__global__ __launch_bounds__(256) void k_fm_graph_state(VIndex V, const u64 *__restrict__ text, const u64 *__restrict__ coff,
                                                        const FmOvlRec *__restrict__ table, u64 nrec, u8 *__restrict__ state) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrec) return;
    const u64 a0 = coff[i] + i, m = coff[i + 1] - coff[i];
    u64 lo = 0, hi = V.n;
    for (u64 k = m; k > 0 && lo < hi; k--) {
        const u32 s = text_symbol(text, a0 + k - 1);
        u64 ol, oh;
        fm_occ2(V, s, lo, hi, &ol, &oh);
        lo = V.C[s] + ol; hi = V.C[s] + oh;
    }
    if (hi < lo) hi = lo;
    const u64 a = lower_bound_dev<u64>(V.srows, 0, V.nsep, lo);
    const u64 b = lower_bound_dev<u64>(V.srows, a, V.nsep, hi);
    const u32 ml = (u32)(m < 0xFFFFFFFFull ? m : 0xFFFFFFFFull);
    u64 copies = 0, first = i;
    for (u64 k = a; k < b; k++) {
        const FmOvlRec e = table[k];
        if (e.length == ml) { copies++; if (e.record < first) first = e.record; }
    }
    state[i] = first < i ? 1u : (hi - lo > copies ? 2u : 0u);
}

// Hit t of a chunk is hit g0 + t of the batch, whose sources are records p0 .. p0 + np - 1 with their hits in
// [hbase[s], hbase[s + 1]).  raw[g0 + t]: the hit's (record, length) when the target is kept and is not the source, else
// a gap.  An edge between two kept records that covers one of them whole cannot be: counted in ctr[FM_GR_BADLEN].
__global__ __launch_bounds__(256) void k_fm_graph_pack(const uint4 *__restrict__ hits, u64 g0, u64 count,
                                                       const u64 *__restrict__ hbase, u64 p0, u64 np,
                                                       const u8 *__restrict__ state, FmEdge *__restrict__ raw,
                                                       u64 *__restrict__ ctr) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint4 h = hits[t];
    const u64 src = p0 + fm_graph_segment(hbase, np, g0 + t);
    FmEdge e{FM_GRAPH_GAP, h.y};
    if (h.x != src && state[h.x] == 0) {
        e.record = h.x;
        if (h.w & 3u) atomicAdd((unsigned long long *)&ctr[FM_GR_BADLEN], 1ull);
    }
    raw[g0 + t] = e;
}

// The hits of one source stand in descending length, so the first hit of a record is its longest: flag[g] = 1 for an
// entry that is no gap and whose record no earlier entry of its segment holds.
__global__ __launch_bounds__(256) void k_fm_graph_longest(const FmEdge *__restrict__ raw, const u64 *__restrict__ seg, u64 nseg,
                                                          u64 count, u8 *__restrict__ flag) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    const u32 rec = raw[g].record;
    u8 keep = rec != FM_GRAPH_GAP;
    if (keep)
        for (u64 k = seg[fm_graph_segment(seg, nseg, g)]; k < g; k++)
            if (raw[k].record == rec) { keep = 0; break; }
    flag[g] = keep;
}

__global__ __launch_bounds__(256) void k_fm_graph_degree(const u8 *__restrict__ flag, const u64 *__restrict__ seg, u64 nseg,
                                                         u32 *__restrict__ deg) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    u32 d = 0;
    for (u64 k = seg[s]; k < seg[s + 1]; k++) d += flag[k];
    deg[s] = d;
}

// Entry g of segment s, when flagged, goes to out[oseg[s] + (the flagged entries of s before g)]: order is kept.
__global__ __launch_bounds__(256) void k_fm_graph_scatter(const FmEdge *__restrict__ in, const u8 *__restrict__ flag,
                                                          const u64 *__restrict__ seg, const u64 *__restrict__ oseg, u64 nseg,
                                                          u64 count, FmEdge *__restrict__ out) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count || !flag[g]) return;
    const u64 s = fm_graph_segment(seg, nseg, g);
    u64 o = oseg[s];
    for (u64 k = seg[s]; k < g; k++) o += flag[k];
    out[o] = in[g];
}

// Transitive reduction.  Edge e = (i -> k, L_ik) of source i (its list in descending length) is reducible when an entry
// (i -> j, L_ij) with L_ij > L_ik has (j -> k, |S_j| - L_ij + L_ik) in j's list.  The entries with a larger length are those
// before e's length group; j's list is searched for the first entry of the wanted length (binary, lengths descend) and
// that length group is read through, in whatever record order it stands.  keep[e] = 0 for a reducible edge.  The lists
// are read as they are: no kept bit feeds back, so the result depends on no order of evaluation.
// ctr[FM_GR_LOOKUPS] counts the lists searched, ctr[FM_GR_REDUCIBLE] the edges dropped.
__global__ __launch_bounds__(256) void k_fm_graph_reduce(const u64 *__restrict__ eoff, u64 nnodes, const FmEdge *__restrict__ edges,
                                                         u64 nedges, const u64 *__restrict__ reclen, u8 *__restrict__ keep,
                                                         u64 *__restrict__ ctr) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 lookups = 0, dropped = 0;
    if (e < nedges) {                                          // no early return: the wave sums below need all lanes
        const u64 a = eoff[fm_graph_segment(eoff, nnodes, e)];
        const FmEdge ik = edges[e];
        bool found = false;
        for (u64 t = a; t < e && !found; t++) {
            const FmEdge ij = edges[t];
            if (ij.length <= ik.length) break;
            if (ij.record == ik.record) continue;
            const u64 want = reclen[ij.record] - ij.length + ik.length;
            u64 lo = eoff[ij.record];
            const u64 end = eoff[ij.record + 1];
            u64 hi = end;
            lookups++;
            while (lo < hi) {                                  // first entry with length <= want
                const u64 mid = (lo + hi) >> 1;
                if (edges[mid].length > want) lo = mid + 1; else hi = mid;
            }
            for (; lo < end; lo++) {
                const FmEdge jk = edges[lo];
                if (jk.length != want) break;
                if (jk.record == ik.record) { found = true; break; }
            }
        }
        keep[e] = found ? 0u : 1u;
        dropped = found ? 1 : 0;
    }
    const u64 wl = fm_wave_sum(lookups), wd = fm_wave_sum(dropped);
    if (lane_id() == 0 && (wl | wd)) {
        atomicAdd((unsigned long long *)&ctr[FM_GR_LOOKUPS], (unsigned long long)wl);
        atomicAdd((unsigned long long *)&ctr[FM_GR_REDUCIBLE], (unsigned long long)wd);
    }
}
