// fm_search_kernels.h -- FM-index search with up to K mismatches (substitutions), by mismatch level: a level-L work
// item is (pattern, strand, depth, lo, hi) with L mismatches spent on the pattern's last m - depth characters.  One lane
// takes one item and walks its exact continuation leftwards as k_fm_count does; at every step where the item still has
// mismatch budget it appends each non-empty alternative letter as an item of level L + 1, and at depth 0 with a
// non-empty interval it appends a hit.  The host drains the levels in chunks sized to the buffers (debwt_fm_search).
// Single TU: included by debwt_hip.hip only, after fm_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"

#define FM_SEARCH_MAX_LEN 1024u     // longest pattern: depth fits the item's 16-bit field, children per item <= 4 * 1024
#define FM_SEARCH_MAX_K 4u

// item / hit layout: 3 u64 words {lo, hi, meta}; meta = batch-local pattern (bits 0-31) | depth (32-47) | mismatches
// (48-55) | strand (56)
__host__ __device__ __forceinline__ u64 fm_item_meta(u32 pat, u32 depth, u32 mm, u32 strand) {
    return (u64)pat | ((u64)depth << 32) | ((u64)mm << 48) | ((u64)strand << 56);
}

// the 16 words of rank line b into registers: 8 x 16-byte loads
__device__ __forceinline__ void fm_line_load(const VIndex &V, u64 b, u64 line[VB_LINE]) {
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(V.idx + b * VB_LINE);
#pragma unroll
    for (int q = 0; q < VB_LINE / 2; q++) { const ulonglong2 t = src[q]; line[2 * q] = t.x; line[2 * q + 1] = t.y; }
}

// rows of codes 1..3 among rows [0, off) of the line's 12 words (code 0: off minus the three): branch-free, one partial
// mask per offset
__device__ __forceinline__ void fm_line_codes(const u64 line[VB_LINE], u32 off, u32 c[3]) {
    const u32 q = off >> 5, r = off & 31u;                     // whole words before off, rows of the partial word
    const u64 part = r ? 0x5555555555555555ull << (2 * (32 - r)) : 0ull;
    u32 c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (u32 w = 0; w < VB_WORDS; w++) {
        const u64 valid = w < q ? 0x5555555555555555ull : w == q ? part : 0ull;
        const u64 x = line[4 + w], lb = x & valid, hb = (x >> 1) & valid;
        c1 += (u32)__popcll(lb & ~hb);
        c2 += (u32)__popcll(hb & ~lb);
        c3 += (u32)__popcll(hb & lb);
    }
    c[0] = c1; c[1] = c2; c[2] = c3;
}

// occ(c, i) for c = 0..3 from the counts of fm_line_codes, with fm_occ2's separator correction for code 3
__device__ __forceinline__ void fm_line_occ4(const VIndex &V, const u64 line[VB_LINE], u64 i, u32 off, const u32 c[3],
                                             u64 out[4]) {
    u64 sep;
    if (line[2] >> 40) sep = lower_bound_dev<u64>(V.srows, 0, V.nsep, i);    // 'T' rows = code-3 rows minus separators
    else sep = ((line[0] >> 40) & 0xFFFFFFull) | (((line[1] >> 40) & 0xFFFFFFull) << 24);
    out[0] = (line[0] & VCNT_MASK) + (off - c[0] - c[1] - c[2]);
    out[1] = (line[1] & VCNT_MASK) + c[0];
    out[2] = (line[2] & VCNT_MASK) + c[1];
    out[3] = (line[3] & VCNT_MASK) + c[2] - sep;
}

// occ(c, i) for c = 0..3 and one row i <= n
__device__ __forceinline__ void fm_occ4_one(const VIndex &V, u64 i, u64 out[4]) {
    const u64 b = i / VB_ROWS;
    const u32 off = (u32)(i - b * VB_ROWS);
    u64 line[VB_LINE];
    u32 c[3];
    fm_line_load(V, b, line);
    fm_line_codes(line, off, c);
    fm_line_occ4(V, line, i, off, c, out);
}

// occ(c, lo) and occ(c, hi) for c = 0..3.  When lo and hi share a 384-row line (as soon as the interval is narrow) the
// line is read once and both offsets are counted from the same registers.  Returns the lines read.
__device__ __forceinline__ u32 fm_occ4(const VIndex &V, u64 lo, u64 hi, u64 olo[4], u64 ohi[4]) {
    const u64 b = lo / VB_ROWS;
    if (hi / VB_ROWS != b) { fm_occ4_one(V, lo, olo); fm_occ4_one(V, hi, ohi); return 2u; }
    u64 line[VB_LINE];
    fm_line_load(V, b, line);
    const u32 offl = (u32)(lo - b * VB_ROWS), offh = (u32)(hi - b * VB_ROWS);
    u32 cl[3], ch[3];
    fm_line_codes(line, offl, cl);
    fm_line_codes(line, offh, ch);
    fm_line_occ4(V, line, lo, offl, cl, olo);
    fm_line_occ4(V, line, hi, offh, ch, ohi);
    return 1u;
}

// Wave-aggregated append of cnt (0..7) slots to the counter at ctr: three ballots give every lane its prefix, one lane
// adds the wave's total.  Returns the lane's first slot; the counter counts every slot asked for, also past a buffer's
// capacity, so the host sees an overflow and re-runs the chunk in smaller pieces.
__device__ __forceinline__ u64 fm_wave_append(u64 *ctr, u32 cnt) {
    const u64 b0 = __ballot(cnt & 1u), b1 = __ballot(cnt & 2u), b2 = __ballot(cnt & 4u);
    const u32 tot = (u32)__popcll(b0) + 2u * (u32)__popcll(b1) + 4u * (u32)__popcll(b2);
    if (!tot) return 0;
    const u64 below = lanemask_lt();
    const u32 pre = (u32)__popcll(b0 & below) + 2u * (u32)__popcll(b1 & below) + 4u * (u32)__popcll(b2 & below);
    const int leader = __ffsll((long long)__ballot(1)) - 1;
    u64 base = 0;
    if ((int)lane_id() == leader) base = atomicAdd((unsigned long long *)ctr, (unsigned long long)tot);
    const u32 blo = (u32)__shfl((int)(u32)base, leader, 64), bhi = (u32)__shfl((int)(u32)(base >> 32), leader, 64);
    return (((u64)bhi << 32) | blo) + pre;
}

// One level of the search.  items_in NULL: level 0, item g = i0 + t is pattern plist[g % nact] (identity when plist is
// NULL) on strand g / nact, depth m, interval [0, n).  Else item i0 + t of items_in.  Children (level + 1 < = kmax) go
// to items_out (capacity out_cap), hits to hits (capacity hit_cap).  ctr: [0] children asked, [1] hits asked, [2] rank
// steps, [3] rank lines read.  Strand 1 is the reverse complement, read from the same bytes.
__global__ __launch_bounds__(256) void k_fm_search(VIndex V, const u8 *__restrict__ chars, const u64 *__restrict__ offsets,
                                                   u64 base, const u32 *__restrict__ plist, u64 nact,
                                                   const u64 *__restrict__ items_in, u64 i0, u64 count, u32 level, u32 kmax,
                                                   u64 *__restrict__ items_out, u64 out_cap, u64 *__restrict__ hits,
                                                   u64 hit_cap, u64 *__restrict__ ctr) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    u32 pat, depth, strand;
    u64 lo, hi;
    if (!items_in) {
        const u64 g = i0 + t;
        strand = g >= nact ? 1u : 0u;
        const u64 j = strand ? g - nact : g;
        pat = plist ? plist[j] : (u32)j;
        depth = (u32)(offsets[pat + 1] - offsets[pat]);
        lo = 0; hi = depth ? V.n : 0;                         // an empty pattern has no hit
    } else {
        const u64 *it = items_in + 3 * (i0 + t);
        lo = it[0]; hi = it[1];
        const u64 meta = it[2];
        pat = (u32)meta; depth = (u32)(meta >> 32) & 0xFFFFu; strand = (u32)(meta >> 56) & 1u;
    }
    const u64 a = offsets[pat] - base, m = offsets[pat + 1] - offsets[pat];
    const bool spawn = level < kmax;
    u64 steps = 0, reads = 0;
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
        if (c > 3) { alive = false; break; }                   // no exact continuation at a non-ACGT character
        const u64 cc = c == 0 ? V.C[0] : c == 1 ? V.C[1] : c == 2 ? V.C[2] : V.C[3];
        const u64 nl = c == 0 ? ol[0] : c == 1 ? ol[1] : c == 2 ? ol[2] : ol[3];
        const u64 nh = c == 0 ? oh[0] : c == 1 ? oh[1] : c == 2 ? oh[2] : oh[3];
        lo = cc + nl; hi = cc + nh;
        alive = lo < hi;
    }
    const u64 slot = fm_wave_append(&ctr[1], alive ? 1u : 0u);
    if (alive && slot < hit_cap) {
        u64 *o = hits + 3 * slot;
        o[0] = lo; o[1] = hi; o[2] = fm_item_meta(pat, 0, level, strand);
    }
    if (steps) { atomicAdd((unsigned long long *)&ctr[2], (unsigned long long)steps); atomicAdd((unsigned long long *)&ctr[3], (unsigned long long)reads); }
}
