// fm_repeat_kernels.h -- maximal and supermaximal repeats from the kept LCP array (Definition 11 of debwt_hip.h).
//
// Hierarchy.  Level 0 is the kept lcp array.  Entry b of level t + 1 holds (min, max) of entries [b F, (b + 1) F) of level
// t, F = 1 << sh the fanout (2..64, a power of two); n_0 = n, n_{t+1} = ceil(n_t / F), up to the level that has one entry.
// Levels 1 .. T lie behind one another in one buffer of uint2: tree_bytes = 8 (n_1 + .. + n_T), below 8 (n / (F - 1) + T).
// A group of F lanes reduces one node with cross-lane operations; F divides 64, so no group spans two waves.
//
// Search.  One lane per row r, l = lcp[r].  Three nearest-value searches, each one ascent and one descent:
//   left   the nearest p < r with lcp[p] <= l (row 0 holds 0): r represents an interval iff lcp[p] < l, and then i = p;
//   right  the nearest q > r with lcp[q] < l, else n: j = q - 1;
//   above  the nearest q' > r with lcp[q'] > l, else n: no value of (r, j] is above l iff q' >= q.
// The values of (i, r) are above l (r is the first row of (i, j] that holds l), so lcp[i+1 .. j] is flat iff r = i + 1
// and q' >= q; the third search runs only where it decides, for r = i + 1 with no base twice on the left.  The ascent
// reads the entries of the current level up to the end of their node (at most F - 1), steps to the next node of the level
// above where that node lies wholly on the search side, and ends on the first entry that can hold a hit (min <= l,
// min < l, max > l); the descent reads at most F children per level.  At most 2 F reads per level and search, never a
// number that grows with the distance.
//
// Output.  A wave's reported rows are a ballot; the masks go to rmask (and the two flag masks beside it), i and j of a
// reported row to a slot of its own.  k_fm_anc_count and k_fm_anc_scan (the rank of the extract section) turn rmask into
// the rank of every set bit: a row's place in the list, ascending by representative, without a sort and without an
// atomic.  k_fm_rep_write reads the rank lines of the reported rows once more for the left counts.
//
// Scratch of a call beside the tree: 146 u64 (16 counters and the level table) and 16 bytes per workgroup of the search
// (the longest reported repeat of each); a call that writes a list adds 16 n (i and j per row) + 28 ceil(n / 64) (three masks and the prefix per
// wave) + 8 (ceil(n / 16384) + 1) (tile offsets) + 64 bytes per record of the list.  Single TU: included by debwt_hip.hip
// only, after fm_esa_kernels.h.
#pragma once
#include "common.h"
#include "fm_esa_kernels.h"

#define FM_REP_MAXLEV 64                // levels above level 0 at fanout 2 and n < 2^64

// counters of a call (u64 each)
#define FM_REP_C_SEARCHED 0             // rows that passed the skip (capped rows included)
#define FM_REP_C_REPS 1                 // of them, representatives
#define FM_REP_C_CAPPED 2               // representatives whose stored value is the cap
#define FM_REP_C_MAXIMAL 3
#define FM_REP_C_SUPER 4
#define FM_REP_C_REPORTED 5
#define FM_REP_C_STEPS 6                // entries read by the searches, every level
#define FM_REP_C_WAVE 7                 // 64 x the reads of the longest lane of every wave and tile
#define FM_REP_C_LINES 8                // rank lines read for left counts (search kernel)
#define FM_REP_NCTR 16

struct FmRepTree {
    const u32 *lcp;        // level 0, n entries
    const uint2 *node;     // levels 1 .. T; x = min, y = max
    const u64 *lev;        // 2 (T + 1) words: n_t, then the first entry of level t in node (level 0: 0)
    u32 levels, sh;        // T; log2 F
};

struct FmRepOpts {
    u32 min_len, kind, cap;               // cap: the non-zero max_lcp of the build, else 0
    u64 min_occ, max_occ;                 // max_occ 0: no bound
};

// One level: nin entries in, nout = ceil(nin / F) out.  LEAF: the input is the lcp array.
template <bool LEAF>
__global__ __launch_bounds__(256) void k_fm_rep_level(const u32 *__restrict__ lcp, const uint2 *__restrict__ in, u64 nin, u32 sh,
                                                      uint2 *__restrict__ out, u64 nout) {
    const u32 F = 1u << sh;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < nin; base += (u64)gridDim.x * blockDim.x) {
        const u64 k = base + threadIdx.x;
        u32 mn = 0xFFFFFFFFu, mx = 0;
        if (k < nin) {
            if (LEAF) mn = mx = lcp[k];
            else { const uint2 v = in[k]; mn = v.x; mx = v.y; }
        }
        for (u32 d = 1; d < F; d <<= 1) {
            const u32 a = (u32)__shfl_xor((int)mn, (int)d, 64), b = (u32)__shfl_xor((int)mx, (int)d, 64);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if ((threadIdx.x & (F - 1)) == 0 && (k >> sh) < nout) out[k >> sh] = make_uint2(mn, mx);
    }
}

// MODE 0: value <= l somewhere below the entry; 1: value < l; 2: value > l
template <int MODE>
__device__ __forceinline__ bool fm_rep_hit(const FmRepTree &T, const u64 *soff, u32 t, u64 pos, u32 l) {
    u32 mn, mx;
    if (t == 0) mn = mx = T.lcp[pos];
    else { const uint2 v = T.node[soff[t] + pos]; mn = v.x; mx = v.y; }
    return MODE == 0 ? mn <= l : MODE == 1 ? mn < l : mx > l;
}

// the nearest q > r whose value hits, else n.  sn, soff: the level table in LDS.
template <int MODE>
__device__ __forceinline__ u64 fm_rep_right(const FmRepTree &T, const u64 *sn, const u64 *soff, u64 r, u32 l, u64 *steps) {
    const u64 n = sn[0], fm = (1ull << T.sh) - 1;
    u64 pos = r + 1;
    u32 t = 0;
    for (;;) {
        if (pos >= sn[t]) return n;                            // nothing to the right on this level or above
        if ((pos & fm) == 0 && t < T.levels) { pos >>= T.sh; t++; continue; }   // the node above lies wholly to the right
        ++*steps;
        if (fm_rep_hit<MODE>(T, soff, t, pos, l)) break;
        pos++;
    }
    while (t > 0) {                                            // the first child that hits
        t--;
        pos <<= T.sh;
        const u64 end = pos + fm + 1 < sn[t] ? pos + fm + 1 : sn[t];
        for (;;) {
            if (pos >= end) return n;                          // never: the node above said so
            ++*steps;
            if (fm_rep_hit<MODE>(T, soff, t, pos, l)) break;
            pos++;
        }
    }
    return pos;
}

// the nearest p < r with lcp[p] <= l; r >= 1.  ~0 when there is none (never: lcp[0] = 0).
__device__ __forceinline__ u64 fm_rep_left(const FmRepTree &T, const u64 *sn, const u64 *soff, u64 r, u32 l, u64 *steps) {
    const u64 fm = (1ull << T.sh) - 1;
    u64 pos = r - 1;
    u32 t = 0;
    for (;;) {
        if (((pos + 1) & fm) == 0 && t < T.levels) { pos >>= T.sh; t++; continue; }  // the node above lies wholly to the left
        ++*steps;
        if (fm_rep_hit<0>(T, soff, t, pos, l)) break;
        if (pos == 0) return ~0ull;
        pos--;
    }
    while (t > 0) {                                            // the last child that hits
        t--;
        const u64 first = pos << T.sh;
        pos = first + fm < sn[t] ? first + fm : sn[t] - 1;
        for (;;) {
            ++*steps;
            if (fm_rep_hit<0>(T, soff, t, pos, l)) break;
            if (pos == first) return ~0ull;                    // never: the node above said so
            pos--;
        }
    }
    return pos;
}

struct FmRecFilter {
    u64 min_records, max_records;         // max_records 0: no bound
    u32 flags;                            // DEBWT_FM_RECORDS_UNIQUE
};

// the left counts of rows [i, j]: two rank lines per base, the separators by subtraction
__device__ __forceinline__ void fm_rep_left_counts(const VIndex &V, u64 i, u64 j, u64 left[5]) {
    u64 sum = 0;
#pragma unroll
    for (u32 s = 0; s < 4; s++) { left[s] = v_occ(V, s, j + 1) - v_occ(V, s, i); sum += left[s]; }
    left[4] = j - i + 1 - sum;
}

// One lane per row, a tile of 256 rows per workgroup and step of its stride.  lo, hi, rmask, mmask, smask: null for a call
// that only counts.  best: 2 u64 per workgroup, the longest reported length and its row_lo (the lowest on ties).
// REC: the record filter of Definition 12 on top, P the kept prefix of fm_record_kernels.h; without REC nothing of the
// filter is compiled in and P, RF are not read.
template <bool REC>
__global__ __launch_bounds__(256) void k_fm_rep_search(VIndex V, FmRepTree T, FmRepOpts O, u64 *__restrict__ lo, u64 *__restrict__ hi,
                                                       u64 *__restrict__ rmask, u64 *__restrict__ mmask, u64 *__restrict__ smask,
                                                       u64 *__restrict__ ctr, u64 *__restrict__ best, const u64 *__restrict__ P,
                                                       FmRecFilter RF) {
    __shared__ u64 sn[FM_REP_MAXLEV + 1], soff[FM_REP_MAXLEV + 1];
    __shared__ u64 sbest[2][4];
    for (u32 k = threadIdx.x; k <= T.levels; k += blockDim.x) { sn[k] = T.lev[2 * k]; soff[k] = T.lev[2 * k + 1]; }
    __syncthreads();
    const u64 n = sn[0], nw = (n + 63) >> 6;
    u64 searched = 0, reps = 0, capped = 0, maximal = 0, super = 0, reported = 0, steps = 0, wave = 0, lines = 0;
    u64 blen = 0, blo = ~0ull;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n; base += (u64)gridDim.x * blockDim.x) {
        const u64 r = base + threadIdx.x;
        const u32 l = r < n ? T.lcp[r] : 0u;
        u64 mine = 0;
        u32 flags = 0;
        bool rep = false;
        if (l && O.cap && l == O.cap) {                        // an interval of the stored value: counted, not reported
            searched++;
            const u64 p = fm_rep_left(T, sn, soff, r, l, &mine);
            if (p != ~0ull && T.lcp[p] < l) { reps++; capped++; }
            mine++;
        } else if (l && l >= O.min_len) {
            searched++;
            const u64 p = fm_rep_left(T, sn, soff, r, l, &mine);
            mine++;
            if (p != ~0ull && T.lcp[p] < l) {
                reps++;
                const u64 q = fm_rep_right<1>(T, sn, soff, r, l, &mine);
                const u64 i = p, j = q - 1, occ = q - p;
                u64 left[5];
                fm_rep_left_counts(V, i, j, left);
                lines += 8;
                u64 mx = left[0];
#pragma unroll
                for (u32 s = 1; s < 4; s++) mx = left[s] > mx ? left[s] : mx;
                if (mx < occ) { flags |= DEBWT_FM_REPEAT_IS_MAXIMAL; maximal++; }
                // the third search only where its answer decides: the head of the interval, no base twice on the left
                if (r == i + 1 && mx <= 1 && fm_rep_right<2>(T, sn, soff, r, l, &mine) >= q) {
                    flags |= DEBWT_FM_REPEAT_IS_SUPERMAXIMAL; super++;
                }
                rep = occ >= O.min_occ && (!O.max_occ || occ <= O.max_occ) &&
                      (O.kind == DEBWT_FM_REPEAT_INTERVALS ||
                       (flags & (O.kind == DEBWT_FM_REPEAT_MAXIMAL ? DEBWT_FM_REPEAT_IS_MAXIMAL : DEBWT_FM_REPEAT_IS_SUPERMAXIMAL)));
                if constexpr (REC) {
                    if (rep) {                                 // records(i, j + 1) of Definition 12: two reads
                        const u64 recs = occ - (P[j] - P[i]);
                        rep = recs >= RF.min_records && (!RF.max_records || recs <= RF.max_records) &&
                              (!(RF.flags & DEBWT_FM_RECORDS_UNIQUE) || recs == occ);
                    }
                }
                if (rep) {
                    reported++;
                    if (l > blen || (l == blen && i < blo)) { blen = l; blo = i; }
                    if (lo) { lo[r] = i; hi[r] = j; }
                }
            }
        }
        steps += mine;
        u64 wmax = mine;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(wmax, d, 64); wmax = o > wmax ? o : wmax; }
        wave += wmax;                                          // the same in every lane
        if (rmask) {
            const u64 br = __ballot(rep), bm = __ballot(rep && (flags & DEBWT_FM_REPEAT_IS_MAXIMAL)),
                      bs = __ballot(rep && (flags & DEBWT_FM_REPEAT_IS_SUPERMAXIMAL));
            const u64 w = r >> 6;
            if (lane_id() == 0 && w < nw) { rmask[w] = br; mmask[w] = bm; smask[w] = bs; }
        }
    }
    u64 v[8] = {searched, reps, capped, maximal, super, reported, steps, lines};
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] += __shfl_xor(v[k], d, 64);
        const u64 ol = __shfl_xor(blen, d, 64), oo = __shfl_xor(blo, d, 64);
        if (ol > blen || (ol == blen && oo < blo)) { blen = ol; blo = oo; }
    }
    if (lane_id() == 0) {
        const int at[8] = {FM_REP_C_SEARCHED, FM_REP_C_REPS, FM_REP_C_CAPPED, FM_REP_C_MAXIMAL, FM_REP_C_SUPER, FM_REP_C_REPORTED,
                           FM_REP_C_STEPS, FM_REP_C_LINES};
#pragma unroll
        for (int k = 0; k < 8; k++) if (v[k]) atomicAdd(&ctr[at[k]], v[k]);
        if (wave) atomicAdd(&ctr[FM_REP_C_WAVE], wave * 64);
        sbest[0][threadIdx.x >> 6] = blen; sbest[1][threadIdx.x >> 6] = blo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 w = 1; w < blockDim.x >> 6; w++)
            if (sbest[0][w] > blen || (sbest[0][w] == blen && sbest[1][w] < blo)) { blen = sbest[0][w]; blo = sbest[1][w]; }
        best[2 * (u64)blockIdx.x] = blen; best[2 * (u64)blockIdx.x + 1] = blo;
    }
}

// One lane per row: a reported row writes its record at the rank of its bit.  wpre, csum: the rank over rmask in the
// layout of k_fm_anc_count and k_fm_anc_scan.  cap: the records out holds.  recs (with P, the kept prefix of Definition 12;
// null for debwt_fm_repeats): the distinct records of every interval of the list, beside it.
__global__ __launch_bounds__(256) void k_fm_rep_write(VIndex V, const u32 *__restrict__ lcp, u64 n, const u64 *__restrict__ lo,
                                                      const u64 *__restrict__ hi, const u64 *__restrict__ rmask,
                                                      const u64 *__restrict__ mmask, const u64 *__restrict__ smask,
                                                      const u32 *__restrict__ wpre, const u64 *__restrict__ csum,
                                                      debwt_fm_repeat *__restrict__ out, u64 cap,
                                                      const u64 *__restrict__ P, u32 *__restrict__ recs) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (u64)gridDim.x * blockDim.x) {
        const u64 w = r >> 6, bit = 1ull << (r & 63), m = rmask[w];
        if (!(m & bit)) continue;
        const u64 k = csum[w / FM_EX_CHUNK_WORDS] + wpre[w] + (u64)__popcll(m & (bit - 1));
        if (k >= cap) continue;                                // never: cap is the sum of the set bits
        const u64 i = lo[r], j = hi[r];
        debwt_fm_repeat rec;
        rec.row_lo = i; rec.count = j - i + 1;
        u64 left[5];
        fm_rep_left_counts(V, i, j, left);
#pragma unroll
        for (u32 s = 0; s < 5; s++) rec.left[s] = left[s];
        rec.len = lcp[r];
        rec.flags = (mmask[w] & bit ? DEBWT_FM_REPEAT_IS_MAXIMAL : 0u) | (smask[w] & bit ? DEBWT_FM_REPEAT_IS_SUPERMAXIMAL : 0u);
        out[k] = rec;
        if (recs) recs[k] = (u32)(rec.count - (P[j] - P[i]));  // records(i, j + 1), as the search computed it
    }
}
