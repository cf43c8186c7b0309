// fm_bigraph_kernels.h -- the string graph over both strands from the index of the records as they are.  Node 2r + o is
// record r as it stands (o = 0) or reverse-complemented (o = 1); the graph is that of the doubled collection (S_0, rc S_0,
// S_1, ...), which is never built.  (i+ -> j+) and (i- -> j+) come from the unchanged overlap walk on both strands,
// (i+ -> j-) from a seed of min_overlap bases that is located and verified against the text, (i- -> j-) is the mirror of
// (j+ -> i+).  The kernels of fm_overlap_kernels.h, fm_graph_kernels.h and k_fm_locate are launched as they are.
//   k_fm_bigraph_state    one lane per record: backward search of the record and of its reverse complement -> both states, self-rc
//   k_fm_bigraph_seed     one lane per record of a batch: the rows of rc(last min_overlap bases), the run k_fm_locate walks
//   k_fm_bigraph_pack     one lane per expanded walk hit: (2 * record, length) in the slot of its (source, strand), or a gap
//   k_fm_bigraph_tail     one lane per located seed occurrence: the tail-to-tail overlap it stands for, verified, or a gap
//   k_fm_bigraph_longest  one lane per slot: keep the longest entry per (segment, target), the first of equal ones
//   k_fm_bigraph_indeg    one lane per edge of the three found kinds: the mirrors each record will receive
//   k_fm_bigraph_place    one lane per edge of the three found kinds: to its node's list, and the mirror of a ++ edge to its
//   k_fm_bigraph_rank     one lane per edge: to its rank by (length descending, target ascending) inside its node's list
// Single TU: included by debwt_hip.hip only, after fm_graph_kernels.h.
#pragma once
#include "common.h"
#include "fm_graph_kernels.h"

// counters of these kernels (u64 each)
enum { FM_BG_BADLEN = 0, FM_BG_SEEDS = 1, FM_BG_TAILS = 2, FM_BG_NCTR = 8 };

// the order of the 32 two-bit symbols of a text window reversed
__device__ __forceinline__ u64 fm_bigraph_rev2(u64 x) {
    const u64 y = __brevll(x);
    return ((y >> 1) & 0x5555555555555555ull) | ((y & 0x5555555555555555ull) << 1);
}

// the record that holds text position p: the last r with coff[r] + r <= p (coff[r] = the bases before record r)
__device__ __forceinline__ u64 fm_bigraph_record(const u64 *__restrict__ coff, u64 nrec, u64 p) {
    u64 lo = 0, hi = nrec;
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (coff[mid] + mid <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// States of record i over both strands.  [lo, hi) of S_i as in k_fm_graph_state, then [lo, hi) of rc S_i: its last base is
// the complement of S_i's first, so the search reads S_i forwards and complements.  The records of S_i's length that start
// in an interval are the copies of that strand; the copies of rc S_i hold i itself exactly when S_i = rc S_i.
// state[2i]: 1 when a copy of either strand has a smaller number, else 2 when either strand occurs more often than it has
// copies, else 0.  state[2i + 1]: 1 for a self-rc record, else state[2i].  selfrc[i]: 1 for a self-rc record.
__global__ __launch_bounds__(256) void k_fm_bigraph_state(VIndex V, const u64 *__restrict__ text, const u64 *__restrict__ coff,
                                                          const FmOvlRec *__restrict__ table, u64 nrec, u8 *__restrict__ state,
                                                          u8 *__restrict__ selfrc) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrec) return;
    const u64 a0 = coff[i] + i, m = coff[i + 1] - coff[i];
    const u32 ml = (u32)(m < 0xFFFFFFFFull ? m : 0xFFFFFFFFull);
    u64 first = i;
    bool inside = false, self = false;
    for (u32 strand = 0; strand < 2; strand++) {
        u64 lo = 0, hi = V.n;
        for (u64 k = 0; k < m && lo < hi; k++) {
            const u32 s = strand ? 3u - text_symbol(text, a0 + k) : text_symbol(text, a0 + m - 1 - k);
            u64 ol, oh;
            fm_occ2(V, s, lo, hi, &ol, &oh);
            lo = V.C[s] + ol; hi = V.C[s] + oh;
        }
        if (hi < lo) hi = lo;
        const u64 a = lower_bound_dev<u64>(V.srows, 0, V.nsep, lo);
        const u64 b = lower_bound_dev<u64>(V.srows, a, V.nsep, hi);
        u64 copies = 0;
        for (u64 k = a; k < b; k++) {
            const FmOvlRec e = table[k];
            if (e.length != ml) continue;
            copies++;
            if (e.record < first) first = e.record;
            if (strand && e.record == i) self = true;
        }
        if (hi - lo > copies) inside = true;
    }
    const u8 st = first < i ? 1u : (inside ? 2u : 0u);
    state[2 * i] = st;
    state[2 * i + 1] = self ? 1u : st;
    selfrc[i] = self ? 1u : 0u;
}

// Seed of record p0 + j of a batch: X = rc(last min_overlap bases of S), searched backwards, so S's last min_overlap
// bases are read forwards and complemented.  row[j] = first row, cnt[j] = rows (0 for a record that is not kept or is
// shorter than min_overlap).  An occurrence of X at offset o of record t is a candidate tail-to-tail overlap of |S_t| - o.
__global__ __launch_bounds__(256) void k_fm_bigraph_seed(VIndex V, const u64 *__restrict__ text, const u64 *__restrict__ coff,
                                                         const u8 *__restrict__ state, u64 p0, u64 np, u32 min_overlap,
                                                         u64 *__restrict__ row, u64 *__restrict__ cnt, u64 *__restrict__ ctr) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 seeds = 0;
    if (j < np) {                                              // no early return: the wave sum below needs all lanes
        const u64 i = p0 + j, m = coff[i + 1] - coff[i];
        u64 lo = 0, hi = 0;
        if (state[2 * i] == 0 && m >= min_overlap) {
            const u64 a0 = coff[i] + i + (m - min_overlap);
            hi = V.n;
            seeds = 1;
            for (u64 k = 0; k < min_overlap && lo < hi; k++) {
                const u32 s = 3u - text_symbol(text, a0 + k);
                u64 ol, oh;
                fm_occ2(V, s, lo, hi, &ol, &oh);
                lo = V.C[s] + ol; hi = V.C[s] + oh;
            }
            if (hi < lo) hi = lo;
        }
        row[j] = lo; cnt[j] = hi - lo;
    }
    const u64 ws = fm_wave_sum(seeds);
    if (lane_id() == 0 && ws) atomicAdd((unsigned long long *)&ctr[FM_BG_SEEDS], (unsigned long long)ws);
}

// Walk hit t of a chunk is hit g0 + t of the batch; the hits of record p0 + j on strand s are [whb[2j + s], whb[2j + s + 1])
// and go to the slots from rawbase[3j + 2s] on (3j: strand 0, 3j + 1: tail candidates, 3j + 2: strand 1).  A strand-0 hit
// is (i+ -> t+), a strand-1 hit (i- -> t+): (2t, length), or a gap when t is not kept, when it is the source's own node
// (t == i on strand 0), or when the source is self-rc on strand 1 (i- is no node).  ctr[FM_BG_BADLEN] as in k_fm_graph_pack.
__global__ __launch_bounds__(256) void k_fm_bigraph_pack(const uint4 *__restrict__ hits, u64 g0, u64 count,
                                                         const u64 *__restrict__ whb, const u64 *__restrict__ rawbase, u64 p0, u64 np,
                                                         const u8 *__restrict__ state, const u8 *__restrict__ selfrc,
                                                         FmEdge *__restrict__ raw, u64 *__restrict__ ctr) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint4 h = hits[t];
    const u64 w = fm_graph_segment(whb, 2 * np, g0 + t), j = w >> 1, strand = w & 1;
    const u64 src = p0 + j;
    FmEdge e{FM_GRAPH_GAP, h.y};
    if (state[2 * (u64)h.x] == 0 && (strand ? !selfrc[src] : h.x != src)) {
        e.record = 2 * h.x;
        if (h.w & 3u) atomicAdd((unsigned long long *)&ctr[FM_BG_BADLEN], 1ull);
    }
    raw[rawbase[3 * j + 2 * strand] + (g0 + t - whb[w])] = e;
}

// Located occurrence t of a chunk is occurrence g0 + t of the batch; those of record p0 + j's seed are [tbase[j], tbase[j + 1])
// and go to the slots from rawbase[3j + 1] on.  The occurrence stands at offset o of record t: L = |S_t| - o, and
// (i+ -> t-, L) holds iff S_t[o ..) = rc(S_i[|S_i| - L ..)).  The first min_overlap bases are the seed; the others are
// compared 32 at a time, a window of S_t against the reversed, complemented window of S_i that ends where the last one
// began.  A gap when L reaches a whole record, when t is not kept or is self-rc (then the walk finds i+ -> t+), or on a
// mismatch.  t == i is an edge: a read whose tail is its own reverse complement.
__global__ __launch_bounds__(256) void k_fm_bigraph_tail(const u64 *__restrict__ text, const u64 *__restrict__ coff, u64 nrec,
                                                         const u64 *__restrict__ pos, u64 g0, u64 count,
                                                         const u64 *__restrict__ tbase, const u64 *__restrict__ rawbase, u64 p0,
                                                         u64 np, u32 min_overlap, const u8 *__restrict__ state,
                                                         const u8 *__restrict__ selfrc, FmEdge *__restrict__ raw,
                                                         u64 *__restrict__ ctr) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 good = 0;
    if (t < count) {                                           // no early return: the wave sum below needs all lanes
        const u64 g = g0 + t, j = fm_graph_segment(tbase, np, g), i = p0 + j;
        const u64 p = pos[t], r = fm_bigraph_record(coff, nrec, p);
        const u64 si = coff[i] + i, mi = coff[i + 1] - coff[i], sr = coff[r] + r, mr = coff[r + 1] - coff[r];
        const u64 o = p - sr;
        FmEdge e{FM_GRAPH_GAP, 0u};
        if (o + min_overlap <= mr) {                           // always: a seed holds no separator
            const u64 L = mr - o;
            bool ok = L < (mi < mr ? mi : mr) && state[2 * r] == 0 && !selfrc[r];
            // S_t[o + min_overlap + x] against the complement of S_i[|S_i| - min_overlap - 1 - x], x in [0, L - min_overlap)
            for (u64 x = 0; ok && x < L - min_overlap; x += 32) {
                const u64 left = L - min_overlap - x, c = left < 32 ? left : 32;
                const u64 a = text_window(text, p + min_overlap + x);
                const u64 b = text_window(text, si + mi - min_overlap - x - c);
                const u64 want = ~(fm_bigraph_rev2(b) << (2 * (32 - c)));
                ok = ((a ^ want) >> (2 * (32 - c))) == 0;
            }
            if (ok) { e.record = (u32)(2 * r + 1); e.length = (u32)L; good = 1; }
        }
        raw[rawbase[3 * j + 1] + (g - tbase[j])] = e;
    }
    const u64 wg = fm_wave_sum(good);
    if (lane_id() == 0 && wg) atomicAdd((unsigned long long *)&ctr[FM_BG_TAILS], (unsigned long long)wg);
}

// flag[g] = 1 for an entry that is no gap and is the longest of its target in its segment, the first among equal ones.
// The segments of a walk descend in length, where this is k_fm_graph_longest's rule; those of the tail stand in row order.
__global__ __launch_bounds__(256) void k_fm_bigraph_longest(const FmEdge *__restrict__ raw, const u64 *__restrict__ seg, u64 nseg,
                                                            u64 count, u8 *__restrict__ flag) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    const FmEdge e = raw[g];
    u8 keep = e.record != FM_GRAPH_GAP;
    if (keep) {
        const u64 s = fm_graph_segment(seg, nseg, g), end = seg[s + 1];
        for (u64 k = seg[s]; k < end; k++) {
            const FmEdge o = raw[k];
            if (o.record == e.record && (o.length > e.length || (o.length == e.length && k < g))) { keep = 0; break; }
        }
    }
    flag[g] = keep;
}

// A: the found edges, record i's in [aoff[3i], aoff[3i + 3)): ++ then +- then -+.  The ++ edge (i+ -> t+) has the mirror
// (t- -> i-) unless i or t is self-rc: mm[t] counts the mirrors record t's second node receives.
__global__ __launch_bounds__(256) void k_fm_bigraph_indeg(const FmEdge *__restrict__ A, const u64 *__restrict__ aoff, u64 nrec,
                                                          u64 count, const u8 *__restrict__ selfrc, u32 *__restrict__ mm) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    const u64 s = fm_graph_segment(aoff, 3 * nrec, g), i = s / 3;
    if (s % 3) return;
    const u32 t = A[g].record >> 1;
    if (!selfrc[i] && !selfrc[t]) atomicAdd(&mm[t], 1u);
}

// Every edge of A to its node's list in cat, lists laid out by eoff (2 nrec + 1): node 2i holds ++ and +- as they stand
// in A, node 2i + 1 holds -+ and then the mirrors, each at the next free place of its list (cur[t], from 0).  The order
// inside a list is settled by k_fm_bigraph_rank.
__global__ __launch_bounds__(256) void k_fm_bigraph_place(const FmEdge *__restrict__ A, const u64 *__restrict__ aoff, u64 nrec,
                                                          u64 count, const u64 *__restrict__ eoff, const u8 *__restrict__ selfrc,
                                                          u32 *__restrict__ cur, FmEdge *__restrict__ cat) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    const u64 s = fm_graph_segment(aoff, 3 * nrec, g), i = s / 3, kind = s % 3;
    const FmEdge e = A[g];
    if (kind == 2) { cat[eoff[2 * i + 1] + (g - aoff[s])] = e; return; }
    cat[eoff[2 * i] + (g - aoff[3 * i])] = e;
    if (kind == 0) {
        const u64 t = e.record >> 1;
        if (!selfrc[i] && !selfrc[t])
            cat[eoff[2 * t + 1] + (aoff[3 * t + 3] - aoff[3 * t + 2]) + atomicAdd(&cur[t], 1u)] = FmEdge{(u32)(2 * i + 1), e.length};
    }
}

// Entry g of node v's list goes to the place of its rank by (length descending, target ascending): the entries of the
// list before it in that order are counted.  A list names a target once, so the ranks differ.
__global__ __launch_bounds__(256) void k_fm_bigraph_rank(const FmEdge *__restrict__ cat, const u64 *__restrict__ eoff, u64 nnodes,
                                                         u64 count, FmEdge *__restrict__ out) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    const u64 v = fm_graph_segment(eoff, nnodes, g), a = eoff[v], b = eoff[v + 1];
    const FmEdge e = cat[g];
    u64 rank = 0;
    for (u64 k = a; k < b; k++) {
        const FmEdge o = cat[k];
        rank += (o.length > e.length || (o.length == e.length && o.record < e.record)) ? 1u : 0u;
    }
    out[a + rank] = e;
}
