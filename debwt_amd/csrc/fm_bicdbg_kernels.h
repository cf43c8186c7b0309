// fm_bicdbg_kernels.h -- the compacted de Bruijn graph of the indexed collection over both strands (Definition 14 of
// debwt_hip.h), from the index of S alone: the doubled collection is never built.  Rows, pieces, lo, the three row bitmaps
// and their ranks are those of fm_cdbg_kernels.h, and so are the ranking rounds (k_fm_cdbg_init, k_fm_cdbg_jump,
// k_fm_cdbg_cut), which run unchanged over the oriented ids.
//
// Oriented ids.  With P pieces, a present node (a piece that is a node) v has id v; the mirror of a present node whose
// reverse complement does not occur has id P + v; the mirror of a mated v is mate[v].  2 P ids, of which the valid ones
// carry FM_BD_VALID in od[].  The host refuses an index of 2^31 rows or more, so every id is below 2^32 - 1 = NONE.
//
// Mates.  One lane per piece: a present node reads its k bases forward from the text at sa[lo[v]] (one text word per 32
// bases) and searches its reverse complement backward with the complemented bases, k rank steps of fm_occ2, which reads
// one rank line once the interval is narrow.  The interval found is a whole piece: mate[v] is its number.
//
// Degrees.  od[id] holds two 4-bit masks, the last bases of the successors (bits 0-3) and the first bases of the
// predecessors (bits 4-7).  Every forward edge string of S is met once, from its target w: per left base c the piece p
// that holds row C[c] + occ(c, i).  The lane ORs the oriented edge p -> w and its mirror mirror(w) -> mirror(p) into the
// masks of the four ends and stores the predecessor ids; an id with one predecessor base gets the same id from every
// writer, and no other id's entry is read.  An edge string whose reverse complement occurs too sets the same bits twice.
//
// Links.  One lane per oriented id y: link[y] = x iff y has one predecessor base, x = pred[y] one successor base, x != y
// and x != mirror(y); the last clause alone refusing counts a hairpin.  The masks' set bits are the oriented edge strings.
//
// Pairs.  After the ranking st[z].x is the first node of z's chain.  The lowest id of a chain is an atomicMin per chain,
// aggregated inside a wave first; a chain is reported iff its minimum is below that of the chain that holds the mirror
// of its first node, and then that minimum is a present node, w*.  A bitmap over the pieces has one bit at each w*: its
// rank is the unitig number.  A cycle was cut at its lowest id, which for the reported one is w*; the other one of the
// pair is never walked: everything about it is read from the reported one through the mirror.
//
// Edges.  Every forward edge string is met again, and it and its mirror are tested: x -> y is a member link iff link[y] = x
// where y's chain is reported, else iff link[mirror(x)] = mirror(y) where that chain is reported (so the unreported cycle
// is cut where the mirror of the reported cut falls), else it is none.  What is no member link goes out as the key
// (2a + oa) << ub | (2b + ob), staged in LDS, ordered by the stable radix passes; equal neighbours are then dropped
// through a rank over the bitmap of the keys that differ from the one before.  The number of edges is known before:
// oriented edge strings - 2 member links.
//
// Single TU: included by debwt_hip.hip only, after fm_cdbg_kernels.h.
#pragma once
#include "common.h"
#include "fm_cdbg_kernels.h"

#define FM_BD_SUCC 0x0000000Fu
#define FM_BD_PRED 0x000000F0u
#define FM_BD_VALID 0x00000100u
#define FM_BD_REP 0x00000200u           // on a first node: the chain is the reported one of its pair
#define FM_BD_EDGE_STAGE 4096           // edge keys a workgroup stages; a tile of 256 nodes emits at most 2048

// counters of a call (u64 each), behind those of fm_cdbg_kernels.h that the ranking rounds write
#define FM_BD_C_MATED 11
#define FM_BD_C_STEPS 12                // rank steps of the mate search
#define FM_BD_C_HAIRPINS 13
#define FM_BD_C_OESTR 14                // oriented edge strings
#define FM_BD_C_REPORTED 15
#define FM_BD_C_CIRC 16                 // reported unitigs that are circular
#define FM_BD_NCTR 24

__device__ __forceinline__ u32 fm_bd_mirror(u32 x, u32 P, const u32 *__restrict__ mate) {
    if (x >= P) return x - P;
    const u32 m = mate[x];
    return m != FM_DBG_NONE ? m : P + x;
}

// One lane per piece: mate[v], and the valid marks of v and of its mirror id.
__global__ __launch_bounds__(256) void k_fm_bicdbg_mates(VIndex V, const u32 *__restrict__ lo, u32 pieces, const u64 *__restrict__ nodebits,
                                                         FmDbgBits S, const u64 *__restrict__ sa, const u64 *__restrict__ text, u32 k,
                                                         u32 *__restrict__ mate, u32 *__restrict__ od, u64 *__restrict__ ctr) {
    u64 mated = 0, steps = 0, bad = 0;
    for (u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; v < pieces; v += (u64)gridDim.x * blockDim.x) {
        const u64 i = lo[v];
        u32 m = FM_DBG_NONE, mark = 0;
        if (fm_dbg_bit(nodebits, i)) {
            mark = FM_BD_VALID;
            const u64 p = sa[i];
            u64 a = 0, b = V.n, word = 0;
            for (u32 j = 0; j < k && a < b; j++) {
                const u64 q = p + j;
                if (j == 0 || (q & 31) == 0) word = text[q >> 5];
                const u32 s = 3u - ((u32)(word >> (((u32)(31 - (q & 31))) << 1)) & 3u);
                u64 ol, oh;
                fm_occ2(V, s, a, b, &ol, &oh);
                a = V.C[s] + ol; b = V.C[s] + oh;
                steps++;
            }
            if (a < b) {
                m = b <= V.n ? fm_dbg_rank(S, a + 1) - 1u : FM_DBG_NONE;
                if (m >= pieces || lo[m] != a || lo[m + 1] != b || !fm_dbg_bit(nodebits, a) || m == (u32)v) { m = FM_DBG_NONE; bad++; }
                else mated++;
            }
        }
        mate[v] = m;
        od[v] = mark;
        od[pieces + v] = m == FM_DBG_NONE ? mark : 0u;
    }
    u64 sums[3] = {mated, steps, bad};
    const int at[3] = {FM_BD_C_MATED, FM_BD_C_STEPS, FM_DBG_C_BAD};
    fm_dbg_block_add<3>(sums, at, ctr);
}

// One lane per piece: a present node w adds every edge string that ends in it, and the mirror of each, to the masks.
__global__ __launch_bounds__(256) void k_fm_bicdbg_degrees(VIndex V, const u32 *__restrict__ lo, u32 pieces, const u64 *__restrict__ nodebits,
                                                           FmDbgBits S, const u64 *__restrict__ sa, const u64 *__restrict__ text, u32 k,
                                                           const u32 *__restrict__ mate, u32 *__restrict__ od, u32 *__restrict__ pred,
                                                           u64 *__restrict__ ctr) {
    u64 lines = 0, bad = 0;
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < pieces; w += (u64)gridDim.x * blockDim.x) {
        const u64 i = lo[w], e = lo[w + 1];
        if (!fm_dbg_bit(nodebits, i)) continue;
        u64 ol[4], oh[4];
        lines += fm_occ4(V, i, e, ol, oh);
        const u32 bw = text_symbol(text, sa[i] + k - 1);       // the last base of w
        const u32 mw = fm_bd_mirror((u32)w, pieces, mate);
#pragma unroll
        for (u32 c = 0; c < 4; c++) {
            if (oh[c] <= ol[c]) continue;
            const u64 row = V.C[c] + ol[c];
            const u32 p = row < V.n ? fm_dbg_rank(S, row + 1) - 1u : FM_DBG_NONE;
            if (p >= pieces || !fm_dbg_bit(nodebits, lo[p])) { bad++; continue; }
            const u32 mp = fm_bd_mirror(p, pieces, mate);
            atomicOr(&od[p], 1u << bw);                        // p -> w
            atomicOr(&od[w], 16u << c);
            pred[w] = p;
            atomicOr(&od[mw], 1u << (3u - c));                 // mirror(w) -> mirror(p)
            atomicOr(&od[mp], 16u << (3u - bw));
            pred[mp] = mw;
        }
    }
    u64 sums[2] = {lines, bad};
    const int at[2] = {FM_DBG_C_LINES, FM_DBG_C_BAD};
    fm_dbg_block_add<2>(sums, at, ctr);
}

// One lane per oriented id: link[y] = pred[y] iff the rule of Definition 14 holds, in place.
__global__ __launch_bounds__(256) void k_fm_bicdbg_links(const u32 *__restrict__ od, const u32 *__restrict__ mate, u32 *__restrict__ link,
                                                         u8 *__restrict__ hasnext, u32 pieces, u64 *__restrict__ ctr) {
    u64 links = 0, hairpins = 0, oestr = 0, bad = 0;
    const u64 ids = 2ull * pieces;
    for (u64 y = (u64)blockIdx.x * blockDim.x + threadIdx.x; y < ids; y += (u64)gridDim.x * blockDim.x) {
        const u32 d = od[y];
        u32 l = FM_DBG_NONE;
        if (d & FM_BD_VALID) {
            oestr += (u64)__popc(d & FM_BD_SUCC);
            if (__popc(d & FM_BD_PRED) == 1) {
                const u32 x = link[y];
                if (x >= ids || !(od[x] & FM_BD_VALID)) bad++;
                else if (__popc(od[x] & FM_BD_SUCC) == 1 && x != (u32)y) {
                    if (x == fm_bd_mirror((u32)y, pieces, mate)) hairpins++;
                    else { l = x; hasnext[x] = 1; links++; }
                }
            }
        } else if (d) bad++;                                   // an edge into an id that is none
        link[y] = l;
    }
    u64 sums[4] = {links, hairpins, oestr, bad};
    const int at[4] = {FM_DBG_C_LINKS, FM_BD_C_HAIRPINS, FM_BD_C_OESTR, FM_DBG_C_BAD};
    fm_dbg_block_add<4>(sums, at, ctr);
}

// One lane per oriented id: cmin[first node of the chain] = the lowest id of the chain (cmin is all ones before).
__global__ __launch_bounds__(256) void k_fm_bicdbg_mins(const uint4 *__restrict__ st, const u32 *__restrict__ od, u32 pieces,
                                                        u32 *__restrict__ cmin) {
    const u64 ids = 2ull * pieces;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < ids; base += (u64)gridDim.x * blockDim.x) {
        const u64 z = base + threadIdx.x;
        const bool node = z < ids && (od[z] & FM_BD_VALID);
        const u32 h = node ? st[z].x : 0u;
        u64 todo = __ballot(node);
        while (todo) {                                         // the lanes of a wave that share a chain ask once
            const int leader = __ffsll((long long)todo) - 1;
            const u32 key = (u32)__shfl((int)h, leader, 64);
            const bool mine = node && h == key;
            u32 x = mine ? (u32)z : FM_DBG_NONE;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { const u32 o = (u32)__shfl_xor((int)x, d, 64); x = o < x ? o : x; }
            if ((int)lane_id() == leader) atomicMin(&cmin[key], x);
            todo &= ~__ballot(mine);
        }
    }
}

// One lane per oriented id: a first node marks its chain as reported or not and sets the bit of w*.
__global__ __launch_bounds__(256) void k_fm_bicdbg_pairs(const uint4 *__restrict__ st, u32 *__restrict__ od, const u32 *__restrict__ link,
                                                         const u32 *__restrict__ mate, const u32 *__restrict__ cmin, u32 pieces,
                                                         u64 *__restrict__ wbits, u64 *__restrict__ ctr) {
    u64 reported = 0, circ = 0, bad = 0;
    u32 longest = 0;
    const u64 ids = 2ull * pieces;
    for (u64 h = (u64)blockIdx.x * blockDim.x + threadIdx.x; h < ids; h += (u64)gridDim.x * blockDim.x) {
        const u32 d = od[h];
        if (!(d & FM_BD_VALID)) continue;
        const u32 len = st[h].y + 1u;
        longest = len > longest ? len : longest;
        if (link[h] != FM_DBG_NONE) continue;
        const u32 other = st[fm_bd_mirror((u32)h, pieces, mate)].x;
        const u32 mine = cmin[h], theirs = cmin[other];
        if (mine == theirs || other == (u32)h) { bad++; continue; }
        if (mine > theirs) continue;
        if (mine >= pieces) { bad++; continue; }
        od[h] = d | FM_BD_REP;
        atomicOr(&wbits[mine >> 6], 1ull << (mine & 63));
        reported++;
        if (d & FM_DBG_CIRC) circ++;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const u32 o = (u32)__shfl_xor((int)longest, d, 64); longest = o > longest ? o : longest; }
    if (lane_id() == 0 && longest) atomicMax(&ctr[FM_DBG_C_LONGEST], (u64)longest);
    u64 sums[3] = {reported, circ, bad};
    const int at[3] = {FM_BD_C_REPORTED, FM_BD_C_CIRC, FM_DBG_C_BAD};
    fm_dbg_block_add<3>(sums, at, ctr);
}

// occ W + occ rc W in S of the oriented node z
__device__ __forceinline__ u64 fm_bd_occ(u32 z, u32 P, const u32 *__restrict__ lo, const u32 *__restrict__ mate) {
    if (z >= P) return (u64)lo[z - P + 1] - lo[z - P];
    const u32 m = mate[z];
    return (u64)lo[z + 1] - lo[z] + (m != FM_DBG_NONE ? (u64)lo[m + 1] - lo[m] : 0ull);
}

// One lane per oriented id: the fields of the unitig records but seq_offset, and len[unitig] = nodes + k - 1.
// out is zeroed before: kmer_count is added to.
__global__ __launch_bounds__(256) void k_fm_bicdbg_unitigs(const uint4 *__restrict__ st, const u32 *__restrict__ od, const u32 *__restrict__ mate,
                                                           const u8 *__restrict__ hasnext, const u32 *__restrict__ lo,
                                                           const u32 *__restrict__ cmin, u32 pieces, FmDbgBits W, u64 unitigs, u32 k,
                                                           debwt_fm_unitig *__restrict__ out, u64 *__restrict__ len) {
    const u64 ids = 2ull * pieces;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < ids; base += (u64)gridDim.x * blockDim.x) {
        const u64 z = base + threadIdx.x;
        bool node = false;
        u32 uid = 0;
        u64 occ = 0;
        if (z < ids && (od[z] & FM_BD_VALID)) {
            const uint4 s = st[z];
            const u32 dh = od[s.x];
            if (dh & FM_BD_REP) {
                const u32 ws = cmin[s.x];
                uid = fm_dbg_rank(W, ws);
                node = uid < unitigs;                          // always
                if (node) {
                    occ = fm_bd_occ((u32)z, pieces, lo, mate);
                    if (s.x == (u32)z) { out[uid].row_lo = lo[ws]; out[uid].flags = dh & FM_DBG_CIRC ? DEBWT_FM_CDBG_CIRCULAR : 0u; }
                    if (!hasnext[z]) { out[uid].nodes = s.y + 1u; len[uid] = (u64)s.y + k; }
                }
            }
        }
        u64 todo = __ballot(node);
        while (todo) {                                         // the lanes of a wave that share a unitig add once
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

// One lane per oriented id of a reported chain: a first node writes seq_offset and its k bases, every other node its last
// base.  A member that does not occur in S is read reverse-complemented from its mirror's occurrence.
__global__ __launch_bounds__(256) void k_fm_bicdbg_seq(const uint4 *__restrict__ st, const u32 *__restrict__ od, const u32 *__restrict__ lo,
                                                       const u32 *__restrict__ cmin, u32 pieces, FmDbgBits W, u64 unitigs, u32 k,
                                                       const u64 *__restrict__ P, const u64 *__restrict__ len, const u64 *__restrict__ sa,
                                                       const u64 *__restrict__ text, u64 n, debwt_fm_unitig *__restrict__ out,
                                                       u8 *__restrict__ seq, u64 seq_bytes) {
    const u64 ids = 2ull * pieces;
    for (u64 z = (u64)blockIdx.x * blockDim.x + threadIdx.x; z < ids; z += (u64)gridDim.x * blockDim.x) {
        if (!(od[z] & FM_BD_VALID)) continue;
        const uint4 s = st[z];
        if (!(od[s.x] & FM_BD_REP)) continue;
        const u32 uid = fm_dbg_rank(W, cmin[s.x]);
        if (uid >= unitigs) continue;                          // never
        const bool flip = z >= pieces;
        const u64 off = P[uid] - len[uid], p = sa[lo[flip ? z - pieces : z]];
        if (p + k > n) continue;                               // never: a node has k bases before its separator
        if (s.x == (u32)z) {
            out[uid].seq_offset = off;
            for (u32 j = 0; j < k && off + j < seq_bytes; j++)
                seq[off + j] = (u8)"ACGT"[flip ? 3u - text_symbol(text, p + k - 1 - j) : text_symbol(text, p + j)];
        } else {
            const u64 at = off + (u64)k - 1 + s.y;
            if (at < seq_bytes) seq[at] = (u8)"ACGT"[flip ? 3u - text_symbol(text, p) : text_symbol(text, p + k - 1)];
        }
    }
}

// the oriented unitig 2a + o whose first or last node z is
__device__ __forceinline__ u64 fm_bd_end(u32 z, u32 P, const uint4 *__restrict__ st, const u32 *__restrict__ od, const u32 *__restrict__ mate,
                                         const u32 *__restrict__ cmin, const FmDbgBits &W) {
    const u32 h = st[z].x;
    if (od[h] & FM_BD_REP) return 2ull * fm_dbg_rank(W, cmin[h]);
    const u32 m = cmin[st[fm_bd_mirror(z, P, mate)].x];
    return m < P ? 2ull * fm_dbg_rank(W, m) + 1ull : 1ull;     // never the second: one chain of a pair is reported
}
// x -> y, an oriented edge string, is a member link
__device__ __forceinline__ bool fm_bd_member(u32 x, u32 y, u32 P, const uint4 *__restrict__ st, const u32 *__restrict__ od,
                                             const u32 *__restrict__ mate, const u32 *__restrict__ link) {
    if (od[st[y].x] & FM_BD_REP) return link[y] == x;
    const u32 mx = fm_bd_mirror(x, P, mate);
    if (od[st[mx].x] & FM_BD_REP) return link[mx] == fm_bd_mirror(y, P, mate);
    return false;
}

// One lane per piece: a present node emits, for every edge string that ends in it, the string and its mirror where they
// are no member links.  cap: the keys the buffer holds.
__global__ __launch_bounds__(256) void k_fm_bicdbg_edges(VIndex V, const uint4 *__restrict__ st, const u32 *__restrict__ od,
                                                         const u32 *__restrict__ mate, const u32 *__restrict__ link,
                                                         const u32 *__restrict__ lo, const u32 *__restrict__ cmin, u32 pieces,
                                                         const u64 *__restrict__ nodebits, FmDbgBits S, FmDbgBits W, u32 ub,
                                                         u64 *__restrict__ keys, u64 cap, u64 *__restrict__ ctr) {
    __shared__ u64 skeys[FM_BD_EDGE_STAGE];
    __shared__ u32 scount;
    __shared__ u64 sbase;
    if (threadIdx.x == 0) scount = 0;
    __syncthreads();
    u64 lines = 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x; ; base += (u64)gridDim.x * blockDim.x) {
        const bool last = base >= pieces;                      // the same in every thread
        const u32 have = scount;                               // read between two barriers: the same in every thread
        __syncthreads();
        if (last || have + 8 * 256 > FM_BD_EDGE_STAGE) {       // the stage leaves with one atomic
            if (threadIdx.x == 0) sbase = have ? atomicAdd(&ctr[FM_DBG_C_EDGES], (u64)have) : 0ull;
            __syncthreads();
            for (u32 i = threadIdx.x; i < have; i += blockDim.x)
                if (sbase + i < cap) keys[sbase + i] = skeys[i];
            __syncthreads();
            if (threadIdx.x == 0) scount = 0;
            __syncthreads();
        }
        if (last) break;
        const u64 w = base + threadIdx.x;
        if (w < pieces && fm_dbg_bit(nodebits, lo[w])) {
            const u64 i = lo[w], e = lo[w + 1];
            const u32 mw = fm_bd_mirror((u32)w, pieces, mate);
            u64 ol[4], oh[4];
            lines += fm_occ4(V, i, e, ol, oh);
#pragma unroll
            for (u32 c = 0; c < 4; c++) {
                if (oh[c] <= ol[c]) continue;
                const u64 row = V.C[c] + ol[c];
                if (row >= V.n) continue;                      // never
                const u32 p = fm_dbg_rank(S, row + 1) - 1u;
                if (p >= pieces) continue;                     // never
                const u32 mp = fm_bd_mirror(p, pieces, mate);
                if (!fm_bd_member(p, (u32)w, pieces, st, od, mate, link))
                    skeys[atomicAdd(&scount, 1u)] = (fm_bd_end(p, pieces, st, od, mate, cmin, W) << ub) | fm_bd_end((u32)w, pieces, st, od, mate, cmin, W);
                if (!fm_bd_member(mw, mp, pieces, st, od, mate, link))
                    skeys[atomicAdd(&scount, 1u)] = (fm_bd_end(mw, pieces, st, od, mate, cmin, W) << ub) | fm_bd_end(mp, pieces, st, od, mate, cmin, W);
            }
        }
        __syncthreads();
    }
    u64 sums[1] = {lines};
    const int at[1] = {FM_DBG_C_LINES};
    fm_dbg_block_add<1>(sums, at, ctr);
}

// One lane per sorted key: bit t = the key differs from the one before it.  bits holds (count >> 6) + 1 zeroed words.
__global__ __launch_bounds__(256) void k_fm_bicdbg_uniq(const u64 *__restrict__ keys, u64 count, u64 *__restrict__ bits) {
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < count; base += (u64)gridDim.x * blockDim.x) {
        const u64 t = base + threadIdx.x;
        const bool first = t < count && (t == 0 || keys[t] != keys[t - 1]);
        const u64 b = __ballot(first);
        if (lane_id() == 0 && t < count) bits[t >> 6] = b;
    }
}

// the keys that differ from the one before, in order: cap is the number the count said
__global__ __launch_bounds__(256) void k_fm_bicdbg_edge_out(const u64 *__restrict__ keys, u64 count, FmDbgBits Q, u32 ub, u64 cap,
                                                            debwt_fm_cdbg_edge *__restrict__ out) {
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (u64)gridDim.x * blockDim.x) {
        if (!fm_dbg_bit(Q.bits, t)) continue;
        const u64 key = keys[t], at = fm_dbg_rank(Q, t);
        if (at >= cap) continue;                               // the host compares the rank's total with the count
        debwt_fm_cdbg_edge e;
        e.from = (u32)(key >> ub); e.to = (u32)(key & ((1ull << ub) - 1ull));
        out[at] = e;
    }
}
