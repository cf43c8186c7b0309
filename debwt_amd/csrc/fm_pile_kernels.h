// fm_pile_kernels.h -- pileup of alignments (definition 7 of debwt_hip.h), calls on the table (definition 8) and the
// insertion events behind a call.  The table is position-major: 8 u32 per text position of the window, 32 bytes.
//   k_fm_pile_stage          one lane per 8 read bytes: the reads of a call as 4-bit codes (0..3, 4 for a non-base)
//   k_fm_pile_plan           one lane per alignment: every validity clause of definition 7, the text an alignment
//                            consumes, and the ops and columns of the input
//   k_fm_pile_count_group<G> G lanes per alignment: the ops are read G at a time and their (query, text) starts come from
//                            a scan inside the group; the lanes then take consecutive columns of each op, so one atomic
//                            instruction of a group adds into G neighbouring positions (G x 32 bytes of the table)
//   k_fm_pile_count_lane     one lane per alignment walking its own CIGAR: the A/B and the check of the form above
//   k_fm_pile_call<WRITE>    one lane per position: one 32-byte load, one text_symbol, one call byte; variants are counted
//                            per block, the host sums the counts, and the second pass writes them in position order
//   k_fm_pile_ins<WRITE>     one lane per alignment: the I ops anchored at a listed position, counted, then written
// The strand is applied where a code is read, as fm_mem_code does: strand 1 reads code m - 1 - x and complements it.
// Counters are summed per wave and leave with one atomic per wave and counter.
// Single TU: included by debwt_hip.hip only, after fm_clean_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"
#include "fm_mem_kernels.h"

struct FmPileAln { u64 pattern, tbeg; u32 qbeg, strand; };     // debwt_fm_pile_aln
struct FmPileVar { u64 t; u32 depth, count, ins; u8 ref, call; };   // debwt_fm_variant
struct FmPileIns { u64 t, aln; u32 qpos, len; };               // debwt_fm_ins_event

// counters (u64 each).  PLAN_*: the input as given; EV_*: adds made to the table (inside the window)
enum { FM_PL_BAD = 0, FM_PL_OPS = 1, FM_PL_MCOLS = 2, FM_PL_DBASES = 3, FM_PL_IOPS = 4,
       FM_PL_EV_BASE = 5, FM_PL_EV_OTHER = 6, FM_PL_EV_DEL = 7, FM_PL_EV_INS = 8, FM_PL_NCTR = 16 };
enum { FM_PL_SLOT_DEL = 4, FM_PL_SLOT_INS = 5, FM_PL_SLOT_OTHER = 6 };
#define FM_PL_NO_CALL 5u
#define FM_PL_INS_BIT 0x10u

__global__ __launch_bounds__(256) void k_fm_pile_stage(const u8 *__restrict__ chars, u64 nwords, u32 *__restrict__ codes) {
    const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    const u64 b = reinterpret_cast<const u64 *>(chars)[w];     // the characters are padded to a multiple of 8 bytes
    u32 c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) c |= fm_code((u8)(b >> (8 * k))) << (4 * k);
    codes[w] = c;
}

// code of position x of the query string of a read whose first character is character `base` of the call and whose
// length is m
__device__ __forceinline__ u32 fm_pile_code(const u32 *__restrict__ codes, u64 base, u64 m, u32 strand, u64 x) {
    const u64 i = base + (strand ? m - 1 - x : x);
    const u32 c = (codes[i >> 3] >> (4 * (u32)(i & 7))) & 15u;
    return strand && c < 4 ? 3u - c : c;
}

__device__ __forceinline__ u64 fm_pile_shfl(u64 v, int src, int width) {
    const u32 lo = (u32)__shfl((int)(u32)v, src, width), hi = (u32)__shfl((int)(u32)(v >> 32), src, width);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 fm_pile_shfl_up(u64 v, int d, int width) {
    const u32 lo = (u32)__shfl_up((int)(u32)v, d, width), hi = (u32)__shfl_up((int)(u32)(v >> 32), d, width);
    return ((u64)hi << 32) | lo;
}

// the counters of one lane into ctr[first ..], one atomic per wave and counter; every lane of the wave must arrive
template <int N>
__device__ __forceinline__ void fm_pile_flush(const u64 (&v)[N], u64 *__restrict__ ctr, int first) {
#pragma unroll
    for (int k = 0; k < N; k++) {
        const u64 s = fm_wave_sum(v[k]);
        if (lane_id() == 0 && s) atomicAdd((unsigned long long *)&ctr[first + k], s);
    }
}

// span[g]: the text alignment g consumes.  bad[0] (starts at ~0): the smallest alignment that breaks a clause.
__global__ __launch_bounds__(256) void k_fm_pile_plan(const u64 *__restrict__ offsets, u64 npat, const FmPileAln *__restrict__ alns,
                                                      u64 naln, const u64 *__restrict__ coff, const u32 *__restrict__ cigar, u64 n,
                                                      u64 *__restrict__ span, u64 *__restrict__ ctr) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 c[4] = {0, 0, 0, 0};                                   // ops, M columns, D bases, I ops
    if (g < naln) {
        const FmPileAln A = alns[g];
        const u64 o0 = coff[g], o1 = coff[g + 1];
        bool ok = A.pattern < npat && A.strand <= 1;
        u64 q = 0, t = 0;
        for (u64 o = o0; o < o1 && ok; o++) {
            const u32 op = cigar[o], kind = op & 15u, len = op >> 4;
            if (kind > 2 || !len || ((o == o0 || o + 1 == o1) && kind)) { ok = false; break; }
            if (kind != 2) q += len;
            if (kind != 1) t += len;
            if (kind == 0) c[1] += len; else if (kind == 2) c[2] += len; else c[3]++;
        }
        if (ok) {
            const u64 m = offsets[A.pattern + 1] - offsets[A.pattern];
            ok = (u64)A.qbeg + q <= m && A.tbeg <= n && t <= n - A.tbeg;
        }
        if (ok) { span[g] = t; c[0] = o1 - o0; }
        else { c[1] = c[2] = c[3] = 0; atomicMin((unsigned long long *)&ctr[FM_PL_BAD], g); }
    }
    fm_pile_flush(c, ctr, FM_PL_OPS);
}

// one add of definition 7; returns the adds made (0 outside the window)
__device__ __forceinline__ u32 fm_pile_add(u32 *__restrict__ counts, u64 wbeg, u64 wend, u64 t, u32 slot) {
    if (t < wbeg || t >= wend) return 0;
    atomicAdd(&counts[((t - wbeg) << 3) + slot], 1u);
    return 1;
}

template <int G>
__global__ __launch_bounds__(256) void k_fm_pile_count_group(const u32 *__restrict__ codes, const u64 *__restrict__ offsets,
                                                             const FmPileAln *__restrict__ alns, u64 naln,
                                                             const u64 *__restrict__ coff, const u32 *__restrict__ cigar,
                                                             const u64 *__restrict__ span, u64 wbeg, u64 wend,
                                                             u32 *__restrict__ counts, u64 *__restrict__ ctr) {
    const u64 g = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const u32 l = threadIdx.x & (G - 1);
    u64 ev[4] = {0, 0, 0, 0};
    if (g < naln) {
        const FmPileAln A = alns[g];
        const u64 o0 = coff[g], o1 = coff[g + 1];
        if (o0 < o1 && A.tbeg < wend && A.tbeg + span[g] > wbeg) {
            const u64 base = offsets[A.pattern], m = offsets[A.pattern + 1] - base;
            u64 q = A.qbeg, t = A.tbeg;
            for (u64 c0 = o0; c0 < o1; c0 += G) {              // every bound of this loop is the same in the whole group
                const u32 op = c0 + l < o1 ? cigar[c0 + l] : 0u;
                const u32 kind = op & 15u, len = op >> 4;
                const u64 ql = kind != 2 ? len : 0, tl = kind != 1 ? len : 0;
                u64 qs = ql, ts = tl;
#pragma unroll
                for (int d = 1; d < G; d <<= 1) {
                    const u64 a = fm_pile_shfl_up(qs, d, G), b = fm_pile_shfl_up(ts, d, G);
                    if ((int)l >= d) { qs += a; ts += b; }
                }
                const u64 qstart = q + qs - ql, tstart = t + ts - tl;
                const u32 cnt = (u32)(o1 - c0 < (u64)G ? o1 - c0 : (u64)G);
                for (u32 j = 0; j < cnt; j++) {
                    const u32 k = (u32)__shfl((int)kind, (int)j, G), L = (u32)__shfl((int)len, (int)j, G);
                    const u64 qj = fm_pile_shfl(qstart, (int)j, G), tj = fm_pile_shfl(tstart, (int)j, G);
                    if (k == 0) {
                        for (u32 x = l; x < L; x += G) {
                            const u64 tt = tj + x;
                            if (tt < wbeg || tt >= wend) continue;
                            const u32 c = fm_pile_code(codes, base, m, A.strand, qj + x);
                            const u32 a = fm_pile_add(counts, wbeg, wend, tt, c < 4 ? c : (u32)FM_PL_SLOT_OTHER);
                            ev[0] += c < 4 ? a : 0; ev[1] += c < 4 ? 0 : a;
                        }
                    } else if (k == 2) {
                        for (u32 x = l; x < L; x += G) ev[2] += fm_pile_add(counts, wbeg, wend, tj + x, FM_PL_SLOT_DEL);
                    } else if (l == 0) {
                        ev[3] += fm_pile_add(counts, wbeg, wend, tj - 1, FM_PL_SLOT_INS);   // tj >= 1: an M op came before
                    }
                }
                q += fm_pile_shfl(qs, G - 1, G);
                t += fm_pile_shfl(ts, G - 1, G);
            }
        }
    }
    fm_pile_flush(ev, ctr, FM_PL_EV_BASE);
}

__global__ __launch_bounds__(256) void k_fm_pile_count_lane(const u32 *__restrict__ codes, const u64 *__restrict__ offsets,
                                                            const FmPileAln *__restrict__ alns, u64 naln,
                                                            const u64 *__restrict__ coff, const u32 *__restrict__ cigar,
                                                            const u64 *__restrict__ span, u64 wbeg, u64 wend,
                                                            u32 *__restrict__ counts, u64 *__restrict__ ctr) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 ev[4] = {0, 0, 0, 0};
    if (g < naln) {
        const FmPileAln A = alns[g];
        const u64 o0 = coff[g], o1 = coff[g + 1];
        if (o0 < o1 && A.tbeg < wend && A.tbeg + span[g] > wbeg) {
            const u64 base = offsets[A.pattern], m = offsets[A.pattern + 1] - base;
            u64 q = A.qbeg, t = A.tbeg;
            for (u64 o = o0; o < o1; o++) {
                const u32 op = cigar[o], kind = op & 15u, len = op >> 4;
                if (kind == 0) {
                    for (u32 x = 0; x < len; x++) {
                        const u64 tt = t + x;
                        if (tt < wbeg || tt >= wend) continue;
                        const u32 c = fm_pile_code(codes, base, m, A.strand, q + x);
                        const u32 a = fm_pile_add(counts, wbeg, wend, tt, c < 4 ? c : (u32)FM_PL_SLOT_OTHER);
                        ev[0] += c < 4 ? a : 0; ev[1] += c < 4 ? 0 : a;
                    }
                    q += len; t += len;
                } else if (kind == 2) {
                    for (u32 x = 0; x < len; x++) ev[2] += fm_pile_add(counts, wbeg, wend, t + x, FM_PL_SLOT_DEL);
                    t += len;
                } else {
                    ev[3] += fm_pile_add(counts, wbeg, wend, t - 1, FM_PL_SLOT_INS);
                    q += len;
                }
            }
        }
    }
    fm_pile_flush(ev, ctr, FM_PL_EV_BASE);
}

// Definition 8 at position wbeg + i.  sep: the nrec separator positions, ascending.  The first pass writes calls, ref
// (where given) and the variants of every block of 256 positions into vcnt; the second writes the variants of block b from
// vbase[b] on, in position order.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_fm_pile_call(const u32 *__restrict__ counts, const u64 *__restrict__ text,
                                                      const u64 *__restrict__ sep, u64 nsep, u64 wbeg, u64 W, u32 min_depth,
                                                      u32 min_permille, u8 *__restrict__ calls, u8 *__restrict__ ref_out,
                                                      u32 *__restrict__ vcnt, const u64 *__restrict__ vbase,
                                                      FmPileVar *__restrict__ vars) {
    __shared__ u32 smem[DEBWT_WAVES + 1];
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 isvar = 0;
    FmPileVar v{};
    if (i < W) {
        const u64 t = wbeg + i;
        const uint4 lo = reinterpret_cast<const uint4 *>(counts)[2 * i], hi = reinterpret_cast<const uint4 *>(counts)[2 * i + 1];
        const u32 c[5] = {lo.x, lo.y, lo.z, lo.w, hi.x};
        const u64 s = lower_bound_dev(sep, 0, nsep, t);
        const u32 ref = s < nsep && sep[s] == t ? 4u : text_symbol(text, t);
        const u64 d = (u64)c[0] + c[1] + c[2] + c[3] + c[4];
        u32 best = 0, cb = c[0];
#pragma unroll
        for (u32 k = 1; k < 5; k++)
            if (c[k] > cb) { best = k; cb = c[k]; }
        const u32 cref = ref == 0 ? c[0] : ref == 1 ? c[1] : ref == 2 ? c[2] : ref == 3 ? c[3] : 0u;
        if (ref < 4 && cref == cb) best = ref;
        const bool called = ref != 4 && d >= min_depth && (u64)cb * 1000 >= (u64)min_permille * d;
        const bool ins = called && (u64)hi.y * 1000 >= (u64)min_permille * d;
        const u32 call = called ? best | (ins ? FM_PL_INS_BIT : 0u) : FM_PL_NO_CALL;
        isvar = called && (best != ref || ins);
        if (!WRITE) {
            calls[i] = (u8)call;
            if (ref_out) ref_out[i] = (u8)ref;
        }
        v.t = t; v.depth = (u32)(d > 0xFFFFFFFFull ? 0xFFFFFFFFull : d); v.count = cb; v.ins = hi.y; v.ref = (u8)ref; v.call = (u8)call;
    }
    if (!WRITE) {
        const u64 b = __ballot(isvar);
        if (lane_id() == 0 && b) atomicAdd(&vcnt[blockIdx.x], (u32)__popcll(b));
    } else {
        u32 total;
        const u32 r = block_scan_excl(isvar, smem, &total);
        if (isvar) vars[vbase[blockIdx.x] + r] = v;
    }
}

// The I ops of alignment g anchored at a position of pos (ascending, npos of them).  Count pass: acnt[g].  Write pass:
// the events of alignment g from abase[g] on, in op order.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_fm_pile_ins(const FmPileAln *__restrict__ alns, u64 naln, const u64 *__restrict__ coff,
                                                     const u32 *__restrict__ cigar, const u64 *__restrict__ span,
                                                     const u64 *__restrict__ pos, u64 npos, u32 *__restrict__ acnt,
                                                     const u64 *__restrict__ abase, FmPileIns *__restrict__ out) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= naln) return;
    const FmPileAln A = alns[g];
    const u64 o0 = coff[g], o1 = coff[g + 1];
    u32 found = 0;
    if (o0 < o1 && npos && A.tbeg <= pos[npos - 1] && A.tbeg + span[g] > pos[0]) {
        u64 q = A.qbeg, t = A.tbeg, w = WRITE ? abase[g] : 0;
        for (u64 o = o0; o < o1; o++) {
            const u32 op = cigar[o], kind = op & 15u, len = op >> 4;
            if (kind == 1) {
                const u64 k = lower_bound_dev(pos, 0, npos, t - 1);
                if (k < npos && pos[k] == t - 1) {
                    if (WRITE) out[w++] = FmPileIns{t - 1, g, (u32)q, len};
                    found++;
                }
            }
            if (kind != 2) q += len;
            if (kind != 1) t += len;
        }
    }
    if (!WRITE) acnt[g] = found;
}
