// fm_extend_kernels.h -- banded affine-gap local alignment of (query, diagonal) jobs against the text of the index.
// The band of a job is the 2w + 1 diagonals k = t - i - diag + w (i: query index, t: text position); with the band
// column c = i + k = t - (diag - w) a cell is (i, c) and its anti-diagonal is a = i + c = 2i + k, so the parity of k is
// the parity of a.  A group of G lanes (16, 32 or 64, G > w) works on one job; lane l owns the diagonal pair (2l, 2l + 1)
// and computes exactly one of the two on every anti-diagonal: no lane of the band idles on alternate steps, and w = 63
// fits the 64 lanes of a wave.  All inputs of a cell were produced one step (left / up neighbour: the other diagonal of
// the lane itself, or the neighbouring lane's, by __shfl_up / __shfl_down inside the group) or two steps earlier (the
// diagonal predecessor: the lane's own register).  The query codes (4 bits each) and the text window of the band
// (m + 2w columns, 2 bits each) are staged in LDS once per job.  Every lane keeps its running maximum and the cell it
// came from; one reduction per job at the end.  With TRACE one byte of direction flags per allowed cell goes to the
// job's slice of a scratch buffer, laid out by (anti-diagonal, lane) so that a step's stores are consecutive bytes;
// k_fm_extend_trace walks it back with one lane per job.
// Single TU: included by debwt_hip.hip only, after fm_mem_kernels.h.
#pragma once
#include "common.h"
#include "fm_mem_kernels.h"

#define FM_EXT_NEG (-(1 << 29))        // "minus infinity": no sum of it and two penalties (<= 510) wraps
#define FM_EXT_MAX_BAND 63
#define FM_EXT_MAX_LEN 65535u

// flag byte of a cell: bits 0-1 where H came from, bit 2 / 3: E / F continued a gap (else opened one), bit 4: mismatch
#define FM_EXT_SRC_START 0u
#define FM_EXT_SRC_DIAG 1u
#define FM_EXT_SRC_E 2u
#define FM_EXT_SRC_F 3u
#define FM_EXT_E_EXT 4u
#define FM_EXT_F_EXT 8u
#define FM_EXT_MISMATCH 16u

struct FmExtJob {
    u64 qoff;            // first byte of the pattern in the batch's characters
    u64 flag_off;        // first flag byte of the job (TRACE)
    long long tbase;     // text position of band column 0 (diag - w); may be negative
    u32 m, strand;
    u32 clo, chi;        // columns [clo, chi) lie inside the job's record
    u32 a0, nsteps;      // first anti-diagonal that holds an allowed cell (even) and the number of anti-diagonals from it
};

// The sampled rows of the index against a text: row i * s holds the symbol before the suffix at sa[i], so its 2-bit
// code in the rank line must be the text's code at sa[i] - 1 (separators are stored as 3 in both).  bad[0]: samples
// that disagree or lie outside the text.
__global__ __launch_bounds__(256) void k_fm_text_check(VIndex V, const u64 *__restrict__ sa, u64 nsamp, u32 sh,
                                                       const u64 *__restrict__ text, u64 *__restrict__ bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsamp) return;
    const u64 p = sa[i], r = i << sh;
    if (p == 0 || r >= V.n) return;
    if (p >= V.n) { atomicAdd((unsigned long long *)bad, 1ull); return; }
    const u64 b = r / VB_ROWS;
    const u32 off = (u32)(r - b * VB_ROWS);
    const u32 s = (u32)(V.idx[b * VB_LINE + 4 + (off >> 5)] >> (2 * (31 - (off & 31)))) & 3u;
    if (s != text_symbol(text, p - 1)) atomicAdd((unsigned long long *)bad, 1ull);
}

// One cell.  hdiag: H(i-1, t-1); hleft, eleft: H and E of (i, t-1); hup, fup: H and F of (i-1, t).  goe = o + e.
// Ties: H takes the diagonal (continuing it only when H(i-1, t-1) > 0, else starting here) before E before F; E and F
// open a new gap rather than continue one.
__device__ __forceinline__ u32 fm_ext_cell(bool ok, u32 q, u32 t, int hdiag, int hleft, int eleft, int hup, int fup,
                                           int sa, int sb, int goe, int ge, int &H, int &E, int &F) {
    const bool eq = q == t;                                    // q = 4 (not a base) equals no text code
    u32 fl = hdiag > 0 ? FM_EXT_SRC_DIAG : FM_EXT_SRC_START;
    int h = (hdiag > 0 ? hdiag : 0) + (eq ? sa : -sb);
    const int eo = hleft - goe, ee = eleft - ge;
    int e = eo;
    if (ee > eo) { e = ee; fl |= FM_EXT_E_EXT; }
    const int fo = hup - goe, fe = fup - ge;
    int f = fo;
    if (fe > fo) { f = fe; fl |= FM_EXT_F_EXT; }
    if (e > h) { h = e; fl = (fl & ~3u) | FM_EXT_SRC_E; }
    if (f > h) { h = f; fl = (fl & ~3u) | FM_EXT_SRC_F; }
    if (!eq) fl |= FM_EXT_MISMATCH;
    H = ok ? h : FM_EXT_NEG; E = ok ? e : FM_EXT_NEG; F = ok ? f : FM_EXT_NEG;
    return fl;
}

// best[j] = score << 32 | (65535 - i) << 8 | (127 - k) of the job's best cell: the largest H, then the smallest query
// index, then the smallest text position (0 in the high word: no positive cell).  cells[j]: allowed cells computed.
// Dynamic LDS: lds_per_job bytes for each of the blockDim.x / G jobs of a workgroup.
template <int G, bool TRACE>
__global__ __launch_bounds__(256) void k_fm_extend(const u64 *__restrict__ text, const u8 *__restrict__ chars,
                                                   const FmExtJob *__restrict__ jobs, u32 njobs, u32 w, int sa, int sb,
                                                   int so, int se, u32 lds_per_job, u8 *__restrict__ flags,
                                                   u64 *__restrict__ best, u32 *__restrict__ cells) {
    extern __shared__ u8 fm_ext_lds[];
    const u32 l = threadIdx.x % G, gi = threadIdx.x / G;
    const u64 j = (u64)blockIdx.x * (blockDim.x / G) + gi;
    FmExtJob J{};                                              // no job: m = 0, no step, nothing allowed
    if (j < njobs) J = jobs[j];
    const int m = (int)J.m, clo = (int)J.clo, chi = (int)J.chi;
    u8 *ql = fm_ext_lds + (size_t)gi * lds_per_job, *tl = ql + ((J.m + 1) >> 1);
    {
        const u8 *p = chars + J.qoff;
        for (u32 x = l; x < (J.m + 1) >> 1; x += G) {
            const u32 c0 = fm_mem_code(p, J.m, J.strand, 2 * x);
            const u32 c1 = 2 * x + 1 < J.m ? fm_mem_code(p, J.m, J.strand, 2 * x + 1) : 4u;
            ql[x] = (u8)(c0 | (c1 << 4));
        }
        const u32 ncol = J.m ? J.m + 2 * w : 0;
        for (u32 x = l; x < (ncol + 3) >> 2; x += G) {
            u32 b = 0;
#pragma unroll
            for (u32 q = 0; q < 4; q++) {
                const int c = (int)(4 * x + q);
                if (c >= clo && c < chi) b |= text_symbol(text, (u64)(J.tbase + c)) << (2 * q);
            }
            tl[x] = (u8)b;
        }
    }
    __syncthreads();
    u32 nst = J.nsteps;                                        // the groups of a wave run the longest job's steps: a uniform loop
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) { const u32 v = (u32)__shfl_xor((int)nst, o, 64); nst = v > nst ? v : nst; }
    const int goe = so + se;
    int He = FM_EXT_NEG, Ee = FM_EXT_NEG, Fe = FM_EXT_NEG, Ho = FM_EXT_NEG, Eo = FM_EXT_NEG, Fo = FM_EXT_NEG;
    int bestS = 0, bestI = 0, bestK = 0;
    u32 ncell = 0;
    u8 *fl_out = flags + J.flag_off + l;
    for (u32 st = 0; st < nst; st += 2) {
        const int half = (int)((J.a0 + st) >> 1);
        const int i = half - (int)l;
        const int qi = i >= 0 && i < m ? i : 0;
        const u32 q = ((u32)ql[qi >> 1] >> ((qi & 1) * 4)) & 15u;
        {                                                      // even anti-diagonal: diagonal 2l, cell (i, half + l)
            const int c = half + (int)l;
            const int hl = __shfl_up(Ho, 1, G), el = __shfl_up(Eo, 1, G);
            const bool ok = l <= w && i >= 0 && i < m && c >= clo && c < chi;
            const int cc = ok ? c : 0;
            const u32 t = ((u32)tl[cc >> 2] >> ((cc & 3) * 2)) & 3u;
            const u32 fl = fm_ext_cell(ok, q, t, He, l ? hl : FM_EXT_NEG, l ? el : FM_EXT_NEG, Ho, Fo, sa, sb, goe, se,
                                       He, Ee, Fe);
            if (ok) {
                ncell++;
                if (TRACE) fl_out[(size_t)st * (w + 1)] = (u8)fl;
                if (He > bestS) { bestS = He; bestI = i; bestK = 2 * (int)l; }
            }
        }
        {                                                      // odd anti-diagonal: diagonal 2l + 1, cell (i, half + l + 1)
            const int c = half + (int)l + 1;
            const int hu = __shfl_down(He, 1, G), fu = __shfl_down(Fe, 1, G);
            const bool ok = l < w && i >= 0 && i < m && c >= clo && c < chi;
            const int cc = ok ? c : 0;
            const u32 t = ((u32)tl[cc >> 2] >> ((cc & 3) * 2)) & 3u;
            const u32 fl = fm_ext_cell(ok, q, t, Ho, He, Ee, l < w ? hu : FM_EXT_NEG, l < w ? fu : FM_EXT_NEG, sa, sb, goe,
                                       se, Ho, Eo, Fo);
            if (ok) {
                ncell++;
                if (TRACE) fl_out[(size_t)(st + 1) * (w + 1)] = (u8)fl;
                if (Ho > bestS) { bestS = Ho; bestI = i; bestK = 2 * (int)l + 1; }
            }
        }
    }
    u64 key = bestS > 0 ? ((u64)(u32)bestS << 32) | ((u64)(65535 - bestI) << 8) | (u64)(127 - bestK) : 0ull;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const u32 lo = (u32)__shfl_xor((int)(u32)key, o, 64), hi = (u32)__shfl_xor((int)(u32)(key >> 32), o, 64);
        const u64 v = ((u64)hi << 32) | lo;
        key = v > key ? v : key;
        ncell += (u32)__shfl_xor((int)ncell, o, 64);
    }
    if (l == 0 && j < njobs) { best[j] = key; cells[j] = ncell; }
}

// Traceback, one lane per job, from the best cell back to the cell whose H started the alignment.  tr[4j ..]: qbeg,
// band column of tbeg, edits (mismatch columns + gap bases), number of CIGAR ops.  ops == NULL: count only; otherwise the
// ops (len << 4 | op, M 0, I 1, D 2) are written from cig_off[j + 1] downwards, so that they read left to right.
__global__ __launch_bounds__(256) void k_fm_extend_trace(const FmExtJob *__restrict__ jobs, u32 njobs, u32 w,
                                                         const u8 *__restrict__ flags, const u64 *__restrict__ best,
                                                         const u64 *__restrict__ cig_off, u32 *__restrict__ ops,
                                                         u32 *__restrict__ tr) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    const u64 key = best[j];
    u32 qbeg = 0, cbeg = 0, edits = 0, nops = 0;
    if (key >> 32) {
        const FmExtJob J = jobs[j];
        int i = 65535 - (int)((key >> 8) & 0xFFFFu), k = 127 - (int)(key & 0xFFu);
        u64 wp = ops ? cig_off[j + 1] : 0;
        const u64 wp0 = ops ? cig_off[j] : 0;
        u32 state = 0, cur = 3, len = 0;                      // state 0: in H, 1: in E (deletion), 2: in F (insertion)
        bool done = false;
        for (u32 guard = 4 * J.m + 4 * w + 8; guard && !done; guard--) {    // columns + state changes of any path
            const int a = 2 * i + k;
            if (i < 0 || i >= (int)J.m || k < 0 || k > 2 * (int)w || a < (int)J.a0 || a >= (int)(J.a0 + J.nsteps)) break;
            const u32 fl = flags[J.flag_off + (size_t)(a - (int)J.a0) * (w + 1) + (u32)(k >> 1)];
            u32 op;
            if (state == 0) {
                const u32 src = fl & 3u;
                if (src == FM_EXT_SRC_E) { state = 1; continue; }
                if (src == FM_EXT_SRC_F) { state = 2; continue; }
                op = 0; edits += (fl >> 4) & 1u;
                qbeg = (u32)i; cbeg = (u32)(i + k);
                if (src == FM_EXT_SRC_START) done = true; else i--;
            } else if (state == 1) {
                op = 2; edits++;
                state = (fl & FM_EXT_E_EXT) ? 1u : 0u;
                k--;                                           // (i, t - 1)
            } else {
                op = 1; edits++;
                state = (fl & FM_EXT_F_EXT) ? 2u : 0u;
                i--; k++;                                      // (i - 1, t)
            }
            if (op == cur) { len++; continue; }
            if (len) { nops++; if (ops && wp > wp0) ops[--wp] = (len << 4) | cur; }
            cur = op; len = 1;
        }
        if (len) { nops++; if (ops && wp > wp0) ops[--wp] = (len << 4) | cur; }
    }
    tr[4 * j] = qbeg; tr[4 * j + 1] = cbeg; tr[4 * j + 2] = edits; tr[4 * j + 3] = nops;
}
