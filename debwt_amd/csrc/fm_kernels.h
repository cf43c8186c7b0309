// fm_kernels.h -- FM-index over the built rows: the rank structure of verify_kernels.h (VIndex, v_occ, v_lf) plus a
// row-sampled suffix array (one u64 text position per row r with r % s == 0), batched backward search (count) and
// LF walks to the nearest sampled row (locate).
// Single TU: included by debwt_hip.hip only, after verify_kernels.h.
#pragma once
#include "common.h"
#include "verify_kernels.h"

// k_vwalk with one store: every current row r of a segment (text position p) with r % s == 0 writes sa[r >> sh] = p.
// Position 0 is no segment's current row: its row (the '$' row) is set by the host.  Same counters as k_vwalk.
__global__ __launch_bounds__(256) void k_fm_walk_samples(VIndex V, const u64 *__restrict__ text, const u64 *__restrict__ sepbits,
                                                         const u64 *__restrict__ bounds, u64 nseg, u32 sh,
                                                         u64 *__restrict__ sa, u64 *__restrict__ counters) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nseg) return;
    const u64 p0 = bounds[2 * j], r0 = bounds[2 * j + 1];
    const u64 smask = (1ull << sh) - 1ull;
    u64 p = bounds[2 * j + 2], r = bounds[2 * j + 3];
    u64 steps = 0;
    bool ok = true;
    while (p > p0) {
        if ((r & smask) == 0 && r < V.n) sa[r >> sh] = p;
        u32 sym;
        const u64 nr = v_lf(V, r, &sym);
        const u32 want = v_text_symbol(text, sepbits, V.n, p - 1);
        if (sym != want) { ok = false; atomicAdd(&counters[0], 1ull); break; }
        r = nr; p--; steps++;
    }
    if (ok && r != r0) { ok = false; atomicAdd(&counters[1], 1ull); }
    if (ok && j == 0) {
        u32 sym;
        (void)v_lf(V, r, &sym);
        if (sym != 5) atomicAdd(&counters[0], 1ull);
    }
    if (steps) atomicAdd(&counters[4], steps);
}

// occ(s, lo) and occ(s, hi) for a base s (0..3).  When both offsets fall in one 384-row line the line is read once
// (8 x 16-byte loads) and counted twice; otherwise the two lines are read independently (both loads in flight).
__device__ __forceinline__ void fm_occ2(const VIndex &V, u32 s, u64 lo, u64 hi, u64 *olo, u64 *ohi) {
    const u64 b = lo / VB_ROWS;
    if (hi / VB_ROWS != b) { *olo = v_occ(V, s, lo); *ohi = v_occ(V, s, hi); return; }
    u64 line[VB_LINE];
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(V.idx + b * VB_LINE);
#pragma unroll
    for (int q = 0; q < VB_LINE / 2; q++) { const ulonglong2 t = src[q]; line[2 * q] = t.x; line[2 * q + 1] = t.y; }
    const u32 offs[2] = {(u32)(lo - b * VB_ROWS), (u32)(hi - b * VB_ROWS)};
    const u64 pat = 0x5555555555555555ull * s;
    const u64 hdr = s == 0 ? line[0] : s == 1 ? line[1] : s == 2 ? line[2] : line[3];   // no dynamic index: stays in VGPRs
    u64 out[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const u32 off = offs[k];
        u64 cnt = hdr & VCNT_MASK;
#pragma unroll
        for (u32 w = 0; w < VB_WORDS; w++) {                   // branch-free over the 12 words: the line is in registers
            const int rem = (int)off - (int)(w * 32);
            const u64 x = line[4 + w] ^ pat;
            u64 m = ~(x | (x >> 1)) & 0x5555555555555555ull;
            if (rem <= 0) m = 0;
            else if (rem < 32) m &= 0x5555555555555555ull << (2 * (32 - rem));
            cnt += (u64)__popcll(m);
        }
        out[k] = cnt;
    }
    if (s == 3) {                                              // 'T' rows = code-3 rows minus the separator rows
        if (line[2] >> 40) {
            out[0] -= lower_bound_dev<u64>(V.srows, 0, V.nsep, lo);
            out[1] -= lower_bound_dev<u64>(V.srows, 0, V.nsep, hi);
        } else {
            const u64 sep_before = ((line[0] >> 40) & 0xFFFFFFull) | (((line[1] >> 40) & 0xFFFFFFull) << 24);
            out[0] -= sep_before; out[1] -= sep_before;
        }
    }
    *olo = out[0]; *ohi = out[1];
}

__device__ __forceinline__ u32 fm_code(u8 ch) {                // A/C/G/T in either case -> 0..3, anything else 4
    switch (ch | 0x20) {
        case 'a': return 0;
        case 'c': return 1;
        case 'g': return 2;
        case 't': return 3;
        default: return 4;
    }
}

// Count: one lane per pattern, backward search over its codes.  chars: the batch's patterns concatenated, offsets[i] -
// base .. offsets[i + 1] - base its bytes.  ranges[2i] = lo, ranges[2i + 1] = hi; an empty pattern or one with a
// character outside ACGTacgt gets lo = hi = 0.
__global__ __launch_bounds__(256) void k_fm_count(VIndex V, const u8 *__restrict__ chars, const u64 *__restrict__ offsets,
                                                  u64 base, u64 npat, u64 *__restrict__ ranges) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npat) return;
    const u64 a = offsets[i] - base, e = offsets[i + 1] - base;
    u64 lo = 0, hi = e > a ? V.n : 0;
    for (u64 k = e; k > a && lo < hi; k--) {
        const u32 s = fm_code(chars[k - 1]);
        if (s > 3) { lo = hi = 0; break; }
        u64 ol, oh;
        fm_occ2(V, s, lo, hi, &ol, &oh);
        lo = V.C[s] + ol; hi = V.C[s] + oh;
    }
    if (hi < lo) hi = lo;
    ranges[2 * i] = lo; ranges[2 * i + 1] = hi;
}

// Locate: one lane per reported occurrence g in [g0, g0 + count).  Runs: run k covers output slots [run_out[k],
// run_out[k + 1]) and rows run_row[k] + (g - run_out[k]); nruns + 1 entries in run_out.  Each lane walks LF until its
// row is sampled: position = (sa[row >> sh] + steps) mod n (the walk may pass the '$' row: LF maps it to row n - 1).
__global__ __launch_bounds__(256) void k_fm_locate(VIndex V, const u64 *__restrict__ sa, u32 sh, const u64 *__restrict__ run_row,
                                                   const u64 *__restrict__ run_out, u64 nruns, u64 g0, u64 count,
                                                   u64 *__restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const u64 g = g0 + t;
    u64 lo = 0, hi = nruns;                                    // last run with run_out[k] <= g
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (run_out[mid] <= g) lo = mid; else hi = mid;
    }
    u64 row = run_row[lo] + (g - run_out[lo]);
    const u64 smask = (1ull << sh) - 1ull;
    u64 steps = 0;
    while ((row & smask) != 0 && steps < V.n) {
        u32 sym;
        row = v_lf(V, row, &sym);
        steps++;
    }
    u64 p = sa[row >> sh] + steps % V.n;
    if (p >= V.n) p -= V.n;
    out[t] = p;
}
