// fm_cdbg_kernels.h -- the compacted de Bruijn graph of the indexed collection, forward strand (Definition 13 of
// debwt_hip.h), from the kept arrays of debwt_fm_esa_build: lcp, sa, da.  Rows, pieces and nodes are below 2^32 (the host
// refuses larger indexes), so every number here is a u32 and NONE = 2^32 - 1 names "no node".
//
// Nodes.  One lane per row writes three bits by ballot: start (lcp[r] < k), node (start and d(sa[r]) >= k) and out (lcp[r]
// <= k and d(sa[r]) >= k + 1: the row begins a (k+1)-interval that is an edge string).  The rank of the extract section
// (k_fm_anc_count, k_fm_anc_scan) over the start bits numbers the pieces in row order, lo[piece] is the piece's first row
// and lo[pieces] = n.  out(W) is a difference of two ranks over the out bits, so a homopolymer's interval of 20,000 rows
// costs what a single row costs.
//
// Degrees.  One lane per piece reads the rank line(s) of its two ends once (fm_occ4): the four left counts.  With one left
// base c the predecessor is the piece that holds row C[c] + occ(c, i), a rank over the start bits.  A second pass keeps
// pred as link iff out(pred) = 1 and pred != v, and marks pred as having a successor; a node is the link of at most one.
//
// Ranking.  Pointer doubling towards the first node over states (anc, dist, mn, md) in two buffers, read from one and
// written to the other: anc is the node dist links before v, mn the lowest node of the span (v, anc] and md its distance.
// A state whose mn is NONE is finished: anc is the first node of the chain and dist the node's rank in it.  Only the
// nodes of a compacted list are visited; a node that finished copies its state to the other buffer in the next round and
// leaves the list, so both buffers hold every finished state and the rounds cost the unfinished nodes alone.  The list
// is written through LDS, 4096 entries per atomic on its counter; its order changes nothing.  On a cycle
// no node finishes; the span of its lowest node m comes back with mn = m, md the cycle's length: m adds md to a counter
// once and keeps the state of one lap.  The host ends the first phase when finished + the lengths of the cycles found =
// the nodes that had a link: an input without cycles ends when its longest chain is ranked.  What is left on the list are
// whole cycles; each m cuts the link into itself, becomes a first node flagged circular, and a second phase ranks the
// list again.  At most ceil(log2(longest)) + 1 rounds a phase.
//
// Unitigs.  The first nodes in piece order are a bitmap; its rank is the unitig number.  The last node writes `nodes`, the
// first row_lo and flags; kmer_count is summed inside a wave over the lanes that share a unitig before one lane adds to
// the unitig (integer adds: the sum does not depend on the order).  seq_offset is a scan of nodes + k - 1 (the scan of the
// records section), every node stores its last base at seq_offset + k - 1 + rank, a first node its k bases.
//
// Edges.  A first node emits from << ub | to for every left base (ub the bits of unitigs - 1); a workgroup stages its keys
// in LDS and takes their slots from a counter with one atomic; the stable radix passes over the 2 ub bits order them, so
// the list does not depend on the order of arrival.
//
// Single TU: included by debwt_hip.hip only, after fm_record_kernels.h.
#pragma once
#include "common.h"
#include "fm_record_kernels.h"
#include "fm_search_kernels.h"

#define FM_DBG_NONE 0xFFFFFFFFu
#define FM_DBG_CIRC 0x80000000u         // in od[v]: the first node of a cycle

// counters of a call (u64 each)
#define FM_DBG_C_NODES 0
#define FM_DBG_C_ESTR 1                 // edge strings: the sum of out()
#define FM_DBG_C_LINKS 2                // links before the cycles are cut
#define FM_DBG_C_LINES 3                // rank lines read
#define FM_DBG_C_BAD 4                  // a left extension whose row lies in no node (never)
#define FM_DBG_C_LIST 5                 // entries of the list being written
#define FM_DBG_C_FIN 6                  // nodes that finished in this phase
#define FM_DBG_C_CYCLEN 7               // the lengths of the cycles found
#define FM_DBG_C_CYCLES 8
#define FM_DBG_C_LONGEST 9
#define FM_DBG_C_EDGES 10               // slots taken by k_fm_cdbg_edges
#define FM_DBG_NCTR 16

// a bitmap with its rank in the layout of k_fm_anc_count and k_fm_anc_scan; one word more than the bits need, so that
// the rank of the position behind the last bit reads a word too
struct FmDbgBits {
    const u64 *bits;
    const u32 *wpre;
    const u64 *csum;
};
// set bits of [0, r)
__device__ __forceinline__ u32 fm_dbg_rank(const FmDbgBits &B, u64 r) {
    const u64 w = r >> 6;
    return (u32)(B.csum[w / FM_EX_CHUNK_WORDS] + B.wpre[w] + (u64)__popcll(B.bits[w] & ((1ull << (r & 63)) - 1ull)));
}
__device__ __forceinline__ bool fm_dbg_bit(const u64 *bits, u64 r) { return (bits[r >> 6] >> (r & 63)) & 1ull; }

#define FM_DBG_CHUNK 4096               // list entries a workgroup stages in LDS before they leave with one atomic
#define FM_DBG_EDGE_STAGE 2048          // edge keys a workgroup stages; a tile of 256 first nodes emits at most 1024

// The survivors of a chunk are gathered in LDS and leave with one atomic on the list's counter.  When every wave took its
// slots with an atomic of its own, the one address served about 28 ns per wave, 1.6 M waves a round on 10^8 nodes: the
// whole time of the round (profiles/r28_fm_cdbg.txt).
struct FmDbgStage { u32 list[FM_DBG_CHUNK]; u32 count; u64 base; };
__device__ __forceinline__ void fm_dbg_stage(bool keep, u32 v, FmDbgStage *st) {
    const u64 m = __ballot(keep);
    if (!m) return;
    u32 base = 0;
    if (lane_id() == 0) base = atomicAdd(&st->count, (u32)__popcll(m));
    base = (u32)__shfl((int)base, 0, 64);
    if (keep) st->list[base + (u32)__popcll(m & lanemask_lt())] = v;
}
// every thread of the workgroup calls it; leaves the stage empty
__device__ __forceinline__ void fm_dbg_flush(FmDbgStage *st, u32 *__restrict__ list, u64 *__restrict__ count) {
    __syncthreads();
    if (threadIdx.x == 0) st->base = st->count ? atomicAdd(count, (u64)st->count) : 0ull;
    __syncthreads();
    const u32 c = st->count;
    const u64 b = st->base;
    for (u32 i = threadIdx.x; i < c; i += blockDim.x) list[b + i] = st->list[i];
    __syncthreads();
    if (threadIdx.x == 0) st->count = 0;
    __syncthreads();
}
// the sums of a workgroup go to the counters with one atomic each: every thread calls it once, at the kernel's end
template <int K>
__device__ __forceinline__ void fm_dbg_block_add(u64 (&v)[K], const int (&at)[K], u64 *__restrict__ ctr) {
    __shared__ u64 sums[K];
    if (threadIdx.x < K) sums[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
        if (lane_id() == 0 && v[k]) atomicAdd(&sums[k], v[k]);
    }
    __syncthreads();
    if (threadIdx.x < K && sums[threadIdx.x]) atomicAdd(&ctr[at[threadIdx.x]], sums[threadIdx.x]);
}

// One lane per row, tiles of 256 rows.  seps: the nrec separator positions.
__global__ __launch_bounds__(256) void k_fm_cdbg_rows(const u32 *__restrict__ lcp, const u64 *__restrict__ sa, const u32 *__restrict__ da,
                                                      const u64 *__restrict__ seps, u64 nrec, u64 n, u32 k,
                                                      u64 *__restrict__ startbits, u64 *__restrict__ nodebits,
                                                      u64 *__restrict__ outbits, u64 *__restrict__ ctr) {
    u64 nodes = 0, estr = 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n; base += (u64)gridDim.x * blockDim.x) {
        const u64 r = base + threadIdx.x;
        bool start = false, node = false, out = false;
        if (r < n) {
            const u32 l = lcp[r], j = da[r];
            const u64 p = sa[r], sp = j < nrec ? seps[j] : 0ull, d = sp > p ? sp - p : 0ull;
            start = l < k;
            node = start && d >= k;
            out = l <= k && d >= (u64)k + 1;
        }
        const u64 bs = __ballot(start), bn = __ballot(node), bo = __ballot(out);
        if (lane_id() == 0 && r < n) {
            startbits[r >> 6] = bs; nodebits[r >> 6] = bn; outbits[r >> 6] = bo;
            nodes += (u64)__popcll(bn); estr += (u64)__popcll(bo);
        }
    }
    if (lane_id() == 0) {
        if (nodes) atomicAdd(&ctr[FM_DBG_C_NODES], nodes);
        if (estr) atomicAdd(&ctr[FM_DBG_C_ESTR], estr);
    }
}

// lo[piece] = the piece's first row; lo[pieces] = n
__global__ __launch_bounds__(256) void k_fm_cdbg_lo(FmDbgBits S, u64 n, u32 pieces, u32 *__restrict__ lo) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (u64)gridDim.x * blockDim.x) {
        if (!fm_dbg_bit(S.bits, r)) continue;
        const u32 p = fm_dbg_rank(S, r);
        if (p < pieces) lo[p] = (u32)r;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) lo[pieces] = (u32)n;
}

// One lane per piece: od = out(W), or NONE for a piece that is no node; pred = the one predecessor, or NONE.
__global__ __launch_bounds__(256) void k_fm_cdbg_degrees(VIndex V, const u32 *__restrict__ lo, u32 pieces,
                                                         const u64 *__restrict__ nodebits, FmDbgBits S, FmDbgBits O,
                                                         u32 *__restrict__ od, u32 *__restrict__ pred, u64 *__restrict__ ctr) {
    u64 lines = 0, bad = 0;
    for (u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; v < pieces; v += (u64)gridDim.x * blockDim.x) {
        const u64 i = lo[v], e = lo[v + 1];
        u32 deg = FM_DBG_NONE, pr = FM_DBG_NONE;
        if (fm_dbg_bit(nodebits, i)) {
            deg = fm_dbg_rank(O, e) - fm_dbg_rank(O, i);
            u64 ol[4], oh[4];
            lines += fm_occ4(V, i, e, ol, oh);
            u32 nin = 0, c = 0;
#pragma unroll
            for (u32 s = 0; s < 4; s++) if (oh[s] > ol[s]) { nin++; c = s; }
            if (nin == 1) {
                u64 row = 0;
#pragma unroll
                for (u32 s = 0; s < 4; s++) if (s == c) row = V.C[s] + ol[s];
                pr = row < V.n ? fm_dbg_rank(S, row + 1) - 1u : FM_DBG_NONE;
                if (pr >= pieces) { pr = FM_DBG_NONE; bad++; }
            }
        }
        od[v] = deg; pred[v] = pr;
    }
    u64 sums[2] = {lines, bad};
    const int at[2] = {FM_DBG_C_LINES, FM_DBG_C_BAD};
    fm_dbg_block_add<2>(sums, at, ctr);
}

// link[v] = pred[v] iff out(pred) = 1 and pred != v, in place: a lane writes its own entry alone and reads od of others
__global__ __launch_bounds__(256) void k_fm_cdbg_links(const u32 *__restrict__ od, u32 *__restrict__ link, u8 *__restrict__ hasnext,
                                                       u32 pieces, u64 *__restrict__ ctr) {
    u64 links = 0, bad = 0;
    for (u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; v < pieces; v += (u64)gridDim.x * blockDim.x) {
        const u32 u = link[v];
        if (u == FM_DBG_NONE) continue;
        const u32 d = od[u];
        if (d == FM_DBG_NONE) bad++;
        if (d == 1u && u != (u32)v) { hasnext[u] = 1; links++; }
        else link[v] = FM_DBG_NONE;
    }
    u64 sums[2] = {links, bad};
    const int at[2] = {FM_DBG_C_LINKS, FM_DBG_C_BAD};
    fm_dbg_block_add<2>(sums, at, ctr);
}

// the states of the first phase, into both buffers; the nodes that have a link go to the list
__global__ __launch_bounds__(256) void k_fm_cdbg_init(const u32 *__restrict__ link, u32 pieces, uint4 *__restrict__ s0,
                                                      uint4 *__restrict__ s1, u32 *__restrict__ list, u64 *__restrict__ ctr) {
    __shared__ FmDbgStage stage;
    if (threadIdx.x == 0) stage.count = 0;
    __syncthreads();
    for (u64 c0 = (u64)blockIdx.x * FM_DBG_CHUNK; c0 < pieces; c0 += (u64)gridDim.x * FM_DBG_CHUNK) {
        for (u32 off = 0; off < FM_DBG_CHUNK && c0 + off < pieces; off += 256) {
            const u64 v = c0 + off + threadIdx.x;
            bool keep = false;
            if (v < pieces) {
                const u32 u = link[v];
                keep = u != FM_DBG_NONE;
                const uint4 s = keep ? make_uint4(u, 1u, u, 1u) : make_uint4((u32)v, 0u, FM_DBG_NONE, 0u);
                s0[v] = s; s1[v] = s;
            }
            fm_dbg_stage(keep, (u32)v, &stage);
        }
        fm_dbg_flush(&stage, list, &ctr[FM_DBG_C_LIST]);
    }
}

// One round: one lane per list entry, states read from `in` and written to `out`.
__global__ __launch_bounds__(256) void k_fm_cdbg_jump(const uint4 *__restrict__ in, uint4 *__restrict__ out,
                                                      const u32 *__restrict__ lin, u64 count, u32 *__restrict__ lout,
                                                      u64 *__restrict__ ctr) {
    __shared__ FmDbgStage stage;
    if (threadIdx.x == 0) stage.count = 0;
    __syncthreads();
    u64 fin = 0, cyclen = 0, cycles = 0;
    for (u64 c0 = (u64)blockIdx.x * FM_DBG_CHUNK; c0 < count; c0 += (u64)gridDim.x * FM_DBG_CHUNK) {
        for (u32 off = 0; off < FM_DBG_CHUNK && c0 + off < count; off += 256) {
            const u64 t = c0 + off + threadIdx.x;
            bool keep = false;
            u32 v = 0;
            if (t < count) {
                v = lin[t];
                const uint4 s = in[v];
                uint4 ns = s;
                if (s.z == FM_DBG_NONE) keep = false;          // finished in the round before: the other buffer gets it too
                else if (s.x == v) keep = true;                // whole laps of a cycle: nothing to add
                else {
                    const uint4 a = in[s.x];
                    keep = true;
                    if (a.z == FM_DBG_NONE) { ns = make_uint4(a.x, s.y + a.y, FM_DBG_NONE, 0u); fin++; }
                    else {
                        ns.x = a.x; ns.y = s.y + a.y;
                        if (a.z < s.z) { ns.z = a.z; ns.w = s.y + a.w; }
                        if (ns.z == v) {                       // the span came back to its lowest node: one lap from here on
                            ns = make_uint4(v, ns.w, v, ns.w);
                            cyclen += ns.w; cycles++;
                        }
                    }
                }
                out[v] = ns;
            }
            fm_dbg_stage(keep, v, &stage);
        }
        fm_dbg_flush(&stage, lout, &ctr[FM_DBG_C_LIST]);
    }
    u64 sums[3] = {fin, cyclen, cycles};
    const int at[3] = {FM_DBG_C_FIN, FM_DBG_C_CYCLEN, FM_DBG_C_CYCLES};
    fm_dbg_block_add<3>(sums, at, ctr);
}

// Between the phases: the list holds whole cycles and the nodes that finished in the last round (they keep their state).
// The lowest node of a cycle (anc = mn = v) cuts the link into itself and becomes a first node; the others start again.
// States into both buffers; cur is one of the two, and a lane reads and writes its own entry alone.
__global__ __launch_bounds__(256) void k_fm_cdbg_cut(const uint4 *cur, u32 *__restrict__ link, u32 *__restrict__ od,
                                                     u8 *__restrict__ hasnext, const u32 *__restrict__ lin, u64 count,
                                                     uint4 *s0, uint4 *s1, u32 *__restrict__ lout, u64 *__restrict__ ctr) {
    __shared__ FmDbgStage stage;
    if (threadIdx.x == 0) stage.count = 0;
    __syncthreads();
    for (u64 c0 = (u64)blockIdx.x * FM_DBG_CHUNK; c0 < count; c0 += (u64)gridDim.x * FM_DBG_CHUNK) {
        for (u32 off = 0; off < FM_DBG_CHUNK && c0 + off < count; off += 256) {
            const u64 t = c0 + off + threadIdx.x;
            bool keep = false;
            u32 v = 0;
            if (t < count) {
                v = lin[t];
                const uint4 s = cur[v];
                const u32 u = link[v];
                uint4 ns;
                if (s.z == FM_DBG_NONE) ns = s;
                else if (s.x == v && s.z == v) {
                    hasnext[u] = 0; link[v] = FM_DBG_NONE; od[v] |= FM_DBG_CIRC;
                    ns = make_uint4(v, 0u, FM_DBG_NONE, 0u);
                } else { ns = make_uint4(u, 1u, u, 1u); keep = true; }
                s0[v] = ns; s1[v] = ns;
            }
            fm_dbg_stage(keep, v, &stage);
        }
        fm_dbg_flush(&stage, lout, &ctr[FM_DBG_C_LIST]);
    }
}

// the first nodes as a bitmap over the pieces, and the longest chain
__global__ __launch_bounds__(256) void k_fm_cdbg_heads(const uint4 *__restrict__ st, const u32 *__restrict__ od,
                                                       const u32 *__restrict__ link, u32 pieces, u64 *__restrict__ headbits,
                                                       u64 *__restrict__ ctr) {
    u32 longest = 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < pieces; base += (u64)gridDim.x * blockDim.x) {
        const u64 v = base + threadIdx.x;
        bool head = false;
        if (v < pieces && od[v] != FM_DBG_NONE) {
            head = link[v] == FM_DBG_NONE;
            const u32 len = st[v].y + 1u;
            longest = len > longest ? len : longest;
        }
        const u64 b = __ballot(head);
        if (lane_id() == 0 && v < pieces) headbits[v >> 6] = b;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const u32 o = (u32)__shfl_xor((int)longest, d, 64); longest = o > longest ? o : longest; }
    if (lane_id() == 0 && longest) atomicMax(&ctr[FM_DBG_C_LONGEST], (u64)longest);
}

// One lane per piece: the fields of the unitig records but seq_offset, and len[unitig] = nodes + k - 1.
// out is zeroed before: kmer_count is added to.
__global__ __launch_bounds__(256) void k_fm_cdbg_unitigs(const uint4 *__restrict__ st, const u32 *__restrict__ od,
                                                         const u32 *__restrict__ link, const u8 *__restrict__ hasnext,
                                                         const u32 *__restrict__ lo, u32 pieces, FmDbgBits H, u64 unitigs, u32 k,
                                                         debwt_fm_unitig *__restrict__ out, u64 *__restrict__ len) {
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < pieces; base += (u64)gridDim.x * blockDim.x) {
        const u64 v = base + threadIdx.x;
        bool node = false;
        u32 uid = 0;
        u64 occ = 0;
        if (v < pieces && od[v] != FM_DBG_NONE) {
            const uint4 s = st[v];
            uid = fm_dbg_rank(H, s.x);
            node = uid < unitigs;                              // always
            if (node) {
                occ = (u64)lo[v + 1] - lo[v];
                if (link[v] == FM_DBG_NONE) { out[uid].row_lo = lo[v]; out[uid].flags = od[v] & FM_DBG_CIRC ? DEBWT_FM_CDBG_CIRCULAR : 0u; }
                if (!hasnext[v]) { out[uid].nodes = s.y + 1u; len[uid] = (u64)s.y + k; }
            }
        }
        // the lanes of a wave that share a unitig add once
        u64 todo = __ballot(node);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const u32 key = (u32)__shfl((int)uid, leader, 64);
            const bool mine = node && uid == key;
            u64 x = mine ? occ : 0ull;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
            if ((int)lane_id() == leader) atomicAdd(reinterpret_cast<u64 *>(&out[key].kmer_count), x);
            todo &= ~__ballot(mine);
        }
    }
}

// One lane per piece: P is the inclusive scan of len.  A first node writes seq_offset and its k bases, every other node its
// last base.  seq holds seq_bytes bytes.
__global__ __launch_bounds__(256) void k_fm_cdbg_seq(const uint4 *__restrict__ st, const u32 *__restrict__ od, const u32 *__restrict__ link,
                                                     const u32 *__restrict__ lo, u32 pieces, FmDbgBits H, u64 unitigs, u32 k,
                                                     const u64 *__restrict__ P, const u64 *__restrict__ len, const u64 *__restrict__ sa,
                                                     const u64 *__restrict__ text, u64 n, debwt_fm_unitig *__restrict__ out,
                                                     u8 *__restrict__ seq, u64 seq_bytes) {
    for (u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; v < pieces; v += (u64)gridDim.x * blockDim.x) {
        if (od[v] == FM_DBG_NONE) continue;
        const uint4 s = st[v];
        const u32 uid = fm_dbg_rank(H, s.x);
        if (uid >= unitigs) continue;                          // never
        const u64 off = P[uid] - len[uid], p = sa[lo[v]];
        if (p + k > n) continue;                               // never: a node has k bases before its separator
        if (link[v] == FM_DBG_NONE) {
            out[uid].seq_offset = off;
            for (u32 j = 0; j < k && off + j < seq_bytes; j++) seq[off + j] = (u8)"ACGT"[text_symbol(text, p + j)];
        } else {
            const u64 at = off + (u64)k - 1 + s.y;
            if (at < seq_bytes) seq[at] = (u8)"ACGT"[text_symbol(text, p + k - 1)];
        }
    }
}

// One lane per piece: a first node emits one key per left base.  cap: the keys the buffer holds.
__global__ __launch_bounds__(256) void k_fm_cdbg_edges(VIndex V, const uint4 *__restrict__ st, const u32 *__restrict__ od,
                                                       const u32 *__restrict__ link, const u32 *__restrict__ lo, u32 pieces,
                                                       FmDbgBits S, FmDbgBits H, u32 ub, u64 *__restrict__ keys, u64 cap,
                                                       u64 *__restrict__ ctr) {
    __shared__ u64 skeys[FM_DBG_EDGE_STAGE];
    __shared__ u32 scount;
    __shared__ u64 sbase;
    if (threadIdx.x == 0) scount = 0;
    __syncthreads();
    u64 lines = 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x; ; base += (u64)gridDim.x * blockDim.x) {
        const bool last = base >= pieces;                      // the same in every thread
        const u32 have = scount;                               // read between two barriers: the same in every thread
        __syncthreads();
        if (last || have + 4 * 256 > FM_DBG_EDGE_STAGE) {      // the stage leaves with one atomic
            if (threadIdx.x == 0) sbase = have ? atomicAdd(&ctr[FM_DBG_C_EDGES], (u64)have) : 0ull;
            __syncthreads();
            for (u32 i = threadIdx.x; i < have; i += blockDim.x)
                if (sbase + i < cap) keys[sbase + i] = skeys[i];
            __syncthreads();
            if (threadIdx.x == 0) scount = 0;
            __syncthreads();
        }
        if (last) break;
        const u64 v = base + threadIdx.x;
        if (v < pieces && od[v] != FM_DBG_NONE && link[v] == FM_DBG_NONE) {
            const u64 i = lo[v], e = lo[v + 1];
            const u64 to = fm_dbg_rank(H, v);
            u64 ol[4], oh[4];
            lines += fm_occ4(V, i, e, ol, oh);
#pragma unroll
            for (u32 c = 0; c < 4; c++) {
                if (oh[c] <= ol[c]) continue;
                const u64 row = V.C[c] + ol[c];
                if (row >= V.n) continue;                      // never
                const u32 u = fm_dbg_rank(S, row + 1) - 1u;
                if (u >= pieces) continue;                     // never
                const u64 from = fm_dbg_rank(H, st[u].x);
                skeys[atomicAdd(&scount, 1u)] = (from << ub) | to;
            }
        }
        __syncthreads();
    }
    u64 sums[1] = {lines};
    const int at[1] = {FM_DBG_C_LINES};
    fm_dbg_block_add<1>(sums, at, ctr);
}

__global__ __launch_bounds__(256) void k_fm_cdbg_edge_out(const u64 *__restrict__ keys, u64 count, u32 ub,
                                                          debwt_fm_cdbg_edge *__restrict__ out) {
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (u64)gridDim.x * blockDim.x) {
        const u64 key = keys[t];
        debwt_fm_cdbg_edge e;
        e.from = (u32)(key >> ub); e.to = (u32)(key & ((1ull << ub) - 1ull));
        out[t] = e;
    }
}
