// fm_clean_kernels.h -- cleaning of a string graph (definition 6 of debwt_hip.h): tips clipped, bubbles popped, in rounds.
// The edge list, the source of every edge and the in-lists (the transpose, as edge numbers) are made once per call and
// stay resident; a round changes only the state bytes, the per-node snapshot and the counters.
//   k_fm_clean_source        one lane per edge: its source, and one more for the in-degree of its target
//   k_fm_clean_transpose     one lane per edge: into the in-list of its target, in whatever order the atomics give
//   k_fm_clean_degree        one lane per node: alive out- and in-degree, first alive successor and predecessor
//   k_fm_clean_tip_mark      one lane per edge: is it alive, a forward tip, a backward tip
//   k_fm_clean_tip_apply     one lane per edge: a tip whose junction keeps another edge gets its chain clipped
//   k_fm_clean_bubble        one lane per node: the branches of a junction that lose their group
//   k_fm_clean_bubble_apply  one lane per edge: a losing branch gets its chain popped
// A node is alive iff its state is 0.  k_fm_clean_degree turns the states into the snapshot of a phase: degrees, and the
// one neighbour of a node of degree 1, so every walk is a chase through succ / pred and reads no list.  The mark and
// bubble kernels read the snapshot only; the apply kernels read the snapshot and the marks and are the only ones that
// write state, so no lane reads what another lane of its launch writes.  A chain has one writer: its first node has one
// alive predecessor (successor, for a backward tip), hence one edge leads into it.
// Single TU: included by debwt_hip.hip only, after fm_bigraph_kernels.h.
#pragma once
#include "common.h"
#include "fm_mem_kernels.h"
#include "fm_graph_kernels.h"

// counters of the cleaning kernels (u64 each), summed over the rounds of a call
enum { FM_CL_TIPS = 0, FM_CL_TIP_NODES = 1, FM_CL_BUBBLES = 2, FM_CL_BUBBLE_NODES = 3, FM_CL_STEPS = 4, FM_CL_NCTR = 8 };
// bits of the per-edge mark byte
enum { FM_CL_TIP_FWD = 1, FM_CL_TIP_BWD = 2, FM_CL_EDGE_ALIVE = 4, FM_CL_LOSER = 8 };
constexpr u32 FM_CL_NODE_CLIPPED = 3, FM_CL_NODE_POPPED = 4;

// the snapshot of a phase
struct FmCleanSnap {
    const u32 *outdeg, *indeg;         // alive degrees; 0 for a node that is not alive
    const u32 *succ, *pred;            // the first alive successor / predecessor in list order: the only one at degree 1
};

__global__ __launch_bounds__(256) void k_fm_clean_source(const u64 *__restrict__ eoff, u64 nnodes, const FmEdge *__restrict__ edges,
                                                         u64 nedges, u32 *__restrict__ src, u32 *__restrict__ incnt) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nedges) return;
    src[e] = (u32)fm_graph_segment(eoff, nnodes, e);
    atomicAdd(&incnt[edges[e].record], 1u);
}

// cur[v] starts at 0; the in-list of v is tin[toff[v] .. toff[v + 1])
__global__ __launch_bounds__(256) void k_fm_clean_transpose(const FmEdge *__restrict__ edges, u64 nedges, const u64 *__restrict__ toff,
                                                            u32 *__restrict__ cur, u64 *__restrict__ tin) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nedges) return;
    const u32 v = edges[e].record;
    tin[toff[v] + atomicAdd(&cur[v], 1u)] = e;
}

__global__ __launch_bounds__(256) void k_fm_clean_degree(const u64 *__restrict__ eoff, const FmEdge *__restrict__ edges,
                                                         const u64 *__restrict__ toff, const u64 *__restrict__ tin,
                                                         const u32 *__restrict__ src, const u8 *__restrict__ state, u64 nnodes,
                                                         u32 *__restrict__ outdeg, u32 *__restrict__ indeg, u32 *__restrict__ succ,
                                                         u32 *__restrict__ pred) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nnodes) return;
    u32 od = 0, id = 0, s = 0, p = 0;
    if (state[v] == 0) {
        for (u64 e = eoff[v]; e < eoff[v + 1]; e++) {
            const u32 t = edges[e].record;
            if (state[t] == 0 && od++ == 0) s = t;
        }
        for (u64 k = toff[v]; k < toff[v + 1]; k++) {
            const u32 t = src[tin[k]];
            if (state[t] == 0 && id++ == 0) p = t;
        }
    }
    outdeg[v] = od; indeg[v] = id; succ[v] = s; pred[v] = p;
}

// The chain c_1 = x, c_2, .. of a tip, forward: indeg 1 at every node, outdeg 1 before the last, outdeg 0 at the last, at
// most max_tip nodes.  Backward is the same on the transposed snapshot, so deg_a / deg_b / next are (indeg, outdeg, succ)
// forward and (outdeg, indeg, pred) backward.  Returns the number of nodes of the tip, 0 when it is none.
__device__ __forceinline__ u32 fm_clean_tip_walk(const u32 *__restrict__ deg_a, const u32 *__restrict__ deg_b,
                                                 const u32 *__restrict__ next, u32 x, u32 max_tip, u64 &steps) {
    u32 c = x;
    for (u32 m = 1; m <= max_tip; m++) {
        steps++;
        if (deg_a[c] != 1) return 0;
        const u32 d = deg_b[c];
        if (d == 0) return m;
        if (d != 1) return 0;
        c = next[c];
    }
    return 0;
}

__global__ __launch_bounds__(256) void k_fm_clean_tip_mark(const FmEdge *__restrict__ edges, const u32 *__restrict__ src, u64 nedges,
                                                           const u8 *__restrict__ state, FmCleanSnap S, u32 max_tip,
                                                           u8 *__restrict__ mark, u64 *__restrict__ ctr) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 steps = 0;
    if (e < nedges) {                                          // no early return: the wave sum below needs all lanes
        const u32 s = src[e], x = edges[e].record;
        u8 m = 0;
        if (state[s] == 0 && state[x] == 0) {
            m = FM_CL_EDGE_ALIVE;
            if (S.outdeg[s] >= 2 && fm_clean_tip_walk(S.indeg, S.outdeg, S.succ, x, max_tip, steps)) m |= FM_CL_TIP_FWD;
            if (S.indeg[x] >= 2 && fm_clean_tip_walk(S.outdeg, S.indeg, S.pred, s, max_tip, steps)) m |= FM_CL_TIP_BWD;
        }
        mark[e] = m;
    }
    const u64 ws = fm_wave_sum(steps);
    if (lane_id() == 0 && ws) atomicAdd((unsigned long long *)&ctr[FM_CL_STEPS], (unsigned long long)ws);
}

// state 3 along the chain of a marked tip; the walk is the one that marked it, so it ends within max_tip.  Returns its nodes.
__device__ __forceinline__ u32 fm_clean_tip_kill(const u32 *__restrict__ deg_b, const u32 *__restrict__ next, u32 x, u32 max_tip,
                                                 u8 *__restrict__ state) {
    u32 c = x, m = 0;
    while (m < max_tip) {
        state[c] = (u8)FM_CL_NODE_CLIPPED;
        m++;
        if (deg_b[c] != 1) break;
        c = next[c];
    }
    return m;
}

__global__ __launch_bounds__(256) void k_fm_clean_tip_apply(const u64 *__restrict__ eoff, const FmEdge *__restrict__ edges,
                                                            const u64 *__restrict__ toff, const u64 *__restrict__ tin,
                                                            const u32 *__restrict__ src, u64 nedges, FmCleanSnap S, u32 max_tip,
                                                            const u8 *__restrict__ mark, u8 *__restrict__ state,
                                                            u64 *__restrict__ ctr) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 tips = 0, nodes = 0;
    if (e < nedges) {
        const u8 m = mark[e];
        const u32 s = src[e], x = edges[e].record;
        if (m & FM_CL_TIP_FWD) {
            bool other = false;                                // an alive edge of the same source that is no tip
            for (u64 k = eoff[s]; k < eoff[s + 1] && !other; k++)
                other = (mark[k] & (FM_CL_EDGE_ALIVE | FM_CL_TIP_FWD)) == FM_CL_EDGE_ALIVE;
            if (other) { tips++; nodes += fm_clean_tip_kill(S.outdeg, S.succ, x, max_tip, state); }
        }
        if (m & FM_CL_TIP_BWD) {
            bool other = false;                                // an alive edge into the same target that is no tip
            for (u64 k = toff[x]; k < toff[x + 1] && !other; k++)
                other = (mark[tin[k]] & (FM_CL_EDGE_ALIVE | FM_CL_TIP_BWD)) == FM_CL_EDGE_ALIVE;
            if (other) { tips++; nodes += fm_clean_tip_kill(S.indeg, S.pred, s, max_tip, state); }
        }
    }
    const u64 wt = fm_wave_sum(tips), wn = fm_wave_sum(nodes);
    if (lane_id() == 0 && wt) {
        atomicAdd((unsigned long long *)&ctr[FM_CL_TIPS], (unsigned long long)wt);
        atomicAdd((unsigned long long *)&ctr[FM_CL_TIP_NODES], (unsigned long long)wn);
    }
}

// The branch that starts with w -> x: nodes of indeg 1 and outdeg 1, at most max_bubble of them, up to a node z of
// indeg >= 2 that is not w.  Returns the number of chain nodes, 0 for no simple branch; z and key (the least chain node,
// shifted by `shift`) are set for a simple branch.
__device__ __forceinline__ u32 fm_clean_branch(const FmCleanSnap &S, u32 w, u32 x, u32 max_bubble, u32 shift, u32 &z, u32 &key,
                                               u64 &steps) {
    u32 c = x, m = 0, k = 0xFFFFFFFFu;
    for (;;) {
        steps++;
        const u32 id = S.indeg[c];
        if (id >= 2) { z = c; key = k; return c != w ? m : 0; }
        if (id == 0 || S.outdeg[c] != 1 || m == max_bubble) return 0;
        m++;
        k = min(k, c >> shift);
        c = S.succ[c];
    }
}

// Edge e of junction w loses iff its branch is simple and, among the simple branches of w that end in the same z, the
// best rank (m descending, key ascending) is held by exactly one branch, which is not e's.
__global__ __launch_bounds__(256) void k_fm_clean_bubble(const u64 *__restrict__ eoff, const FmEdge *__restrict__ edges,
                                                         const u8 *__restrict__ state, u64 nnodes, FmCleanSnap S, u32 max_bubble,
                                                         u32 shift, u8 *__restrict__ mark, u64 *__restrict__ ctr) {
    const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 steps = 0;
    if (w < nnodes) {
        const u64 a = eoff[w], b = eoff[w + 1];
        const bool junction = S.outdeg[w] >= 2;                // 0 for a node that is not alive
        for (u64 e = a; e < b; e++) {
            u8 lose = 0;
            u32 z = 0, key = 0, m = 0;
            if (junction && state[edges[e].record] == 0) m = fm_clean_branch(S, (u32)w, edges[e].record, max_bubble, shift, z, key, steps);
            if (m) {
                u32 bm = m, bk = key, nbest = 1;               // the best rank of the group and how many hold it
                for (u64 j = a; j < b; j++) {
                    if (j == e || state[edges[j].record] != 0) continue;
                    u32 zj = 0, kj = 0;
                    const u32 mj = fm_clean_branch(S, (u32)w, edges[j].record, max_bubble, shift, zj, kj, steps);
                    if (!mj || zj != z) continue;
                    if (mj > bm || (mj == bm && kj < bk)) { bm = mj; bk = kj; nbest = 1; }
                    else if (mj == bm && kj == bk) nbest++;
                }
                lose = nbest == 1 && (bm != m || bk != key);
            }
            mark[e] = lose ? (u8)FM_CL_LOSER : (u8)0;
        }
    }
    const u64 ws = fm_wave_sum(steps);
    if (lane_id() == 0 && ws) atomicAdd((unsigned long long *)&ctr[FM_CL_STEPS], (unsigned long long)ws);
}

__global__ __launch_bounds__(256) void k_fm_clean_bubble_apply(const FmEdge *__restrict__ edges, u64 nedges, FmCleanSnap S,
                                                               u32 max_bubble, const u8 *__restrict__ mark, u8 *__restrict__ state,
                                                               u64 *__restrict__ ctr) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 pops = 0, nodes = 0;
    if (e < nedges && (mark[e] & FM_CL_LOSER)) {
        pops = 1;
        u32 c = edges[e].record;
        while (nodes < max_bubble && S.indeg[c] == 1) {        // the marked walk again: it ends at z within max_bubble
            state[c] = (u8)FM_CL_NODE_POPPED;
            nodes++;
            c = S.succ[c];
        }
    }
    const u64 wp = fm_wave_sum(pops), wn = fm_wave_sum(nodes);
    if (lane_id() == 0 && wp) {
        atomicAdd((unsigned long long *)&ctr[FM_CL_BUBBLES], (unsigned long long)wp);
        atomicAdd((unsigned long long *)&ctr[FM_CL_BUBBLE_NODES], (unsigned long long)wn);
    }
}
