// fm_chain_kernels.h -- banded affine-gap local alignment along a chain of anchors: the band of query row i is centred on
// the diagonal c(i) of the last anchor at or before i, so it shifts from row to row and the anti-diagonal pairs of
// k_fm_extend (a fixed band) do not carry over.  This is a row sweep: a group of G lanes (16, 32 or 64) works on one job
// and steps one query row at a time; lane l owns the band index k = l (and k = l + 64 with S = 2, for w > 31), where
// k = t - i - c(i) + w in 0..2w.  With d = c(i) - c(i-1) the diagonal predecessor of a cell is band index k + d of the row
// before and the upper neighbour k + 1 + d: both come by a variable-lane __shfl of the lane's kept H and F.  The
// dependency along the row is a max-plus prefix scan inside the group: E(i,t) = max over t' < t of Hd(i,t') - o -
// (t - t') e, with Hd the H of a cell without its E term -- exact because o >= 0, so a gap continued out of E never
// beats the same gap continued out of the H that E came from.  One more shuffle of the finished H and E of the left
// neighbour gives the "continued or opened" flag under the tie rule of fm_ext_cell.  The query codes (4 bits each) and,
// where it fits, the text window of all the job's allowed cells (2 bits each) are staged in LDS once per job; a window
// that does not fit is read from the packed text row by row.  With TRACE one byte of flags (the FM_EXT_* coding) per
// band index and row goes to the job's slice of the scratch buffer, 2w + 1 bytes per row, so that a row's stores are
// consecutive; k_fm_chain_trace walks it back with one lane per job.
// Single TU: included by debwt_hip.hip only, after fm_extend_kernels.h.
#pragma once
#include "common.h"
#include "fm_extend_kernels.h"

struct FmChainAnchor {
    u32 q;               // first query row of the anchor's band centre
    int dc;              // its diagonal minus the job's first anchor's
};

struct FmChainJob {
    u64 qoff;            // first byte of the pattern in the batch's characters
    u64 flag_off;        // first flag byte of the job (TRACE)
    u64 aoff;            // first anchor of the job in the batch's anchors
    long long tbase;     // text position of column 0: first anchor's diag - w; column of cell (i, k) = i + dc(i) + k
    u32 m, strand;
    u32 na, a0;          // anchors; the anchor in effect at row i0
    int clo, chi;        // columns [clo, chi) lie inside the job's record
    int wlo;             // first column of the staged text window
    u32 wn;              // its columns (0: not staged, the text is read from memory)
    u32 i0, nrows;       // first query row that holds an allowed cell, rows from it to the last one that does
};

// out[s] = v at band index base + 64 s of the row before (FM_EXT_NEG outside 0..w2)
template <int G, int S>
__device__ __forceinline__ void fm_chain_fetch(const int (&v)[S], int base, int w2, int (&out)[S]) {
    int a[S];
#pragma unroll
    for (int s = 0; s < S; s++) a[s] = __shfl(v[s], base & (G - 1), G);
#pragma unroll
    for (int s = 0; s < S; s++) {
        const int idx = base + 64 * s;
        out[s] = (idx < 0 || idx > w2) ? FM_EXT_NEG : ((S == 2 && (idx >> 6)) ? a[S - 1] : a[0]);
    }
}

// best[j], cells[j] as k_fm_extend writes them (the band index k of the best cell is relative to its row's centre).
// Dynamic LDS: lds_per_job bytes for each of the blockDim.x / G jobs of a workgroup.
template <int G, int S, bool TRACE>
__global__ __launch_bounds__(256) void k_fm_extend_chain(const u64 *__restrict__ text, const u8 *__restrict__ chars,
                                                         const FmChainJob *__restrict__ jobs,
                                                         const FmChainAnchor *__restrict__ anchors, u32 njobs, u32 w, int sa,
                                                         int sb, int so, int se, u32 lds_per_job, u8 *__restrict__ flags,
                                                         u64 *__restrict__ best, u32 *__restrict__ cells) {
    static_assert(S == 1 || G == 64, "two band indices per lane only with a whole wave per job");
    extern __shared__ u8 fm_chain_lds[];
    const u32 l = threadIdx.x % G, gi = threadIdx.x / G;
    const u64 j = (u64)blockIdx.x * (blockDim.x / G) + gi;
    FmChainJob J{};                                            // no job: m = 0, no row, nothing allowed
    if (j < njobs) J = jobs[j];
    const int w2 = 2 * (int)w;
    u8 *ql = fm_chain_lds + (size_t)gi * lds_per_job, *tl = ql + ((J.m + 1) >> 1);
    {
        const u8 *p = chars + J.qoff;
        for (u32 x = l; x < (J.m + 1) >> 1; x += G) {
            const u32 c0 = fm_mem_code(p, J.m, J.strand, 2 * x);
            const u32 c1 = 2 * x + 1 < J.m ? fm_mem_code(p, J.m, J.strand, 2 * x + 1) : 4u;
            ql[x] = (u8)(c0 | (c1 << 4));
        }
        for (u32 x = l; x < (J.wn + 3) >> 2; x += G) {
            u32 b = 0;
#pragma unroll
            for (u32 q = 0; q < 4; q++) {
                const int c = J.wlo + (int)(4 * x + q);
                if (c >= J.clo && c < J.chi) b |= text_symbol(text, (u64)(J.tbase + c)) << (2 * q);
            }
            tl[x] = (u8)b;
        }
    }
    __syncthreads();
    u32 nst = J.nrows;                                         // the groups of a wave run the longest job's rows: a uniform loop
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) { const u32 v = (u32)__shfl_xor((int)nst, o, 64); nst = v > nst ? v : nst; }
    const FmChainAnchor *A = anchors + J.aoff;
    u32 na = J.a0 + 1, qn = ~0u;                               // the next anchor and the row at which it takes over
    int c = 0, dn = 0;
    if (J.na) {
        c = A[J.a0].dc;
        if (na < J.na) { qn = A[na].q; dn = A[na].dc; }
    }
    const int goe = so + se;
    int Hp[S], Fp[S];
#pragma unroll
    for (int s = 0; s < S; s++) Hp[s] = Fp[s] = FM_EXT_NEG;
    int bestS = 0, bestI = 0, bestK = 0;
    u32 ncell = 0;
    u8 *fl_out = flags + J.flag_off + l;
    for (u32 r = 0; r < nst; r++) {
        const bool act = r < J.nrows;
        const int i = (int)(J.i0 + r);
        int dl = 0;
        if (act && (u32)i == qn) {
            dl = dn - c; c = dn; na++;
            if (na < J.na) { qn = A[na].q; dn = A[na].dc; } else qn = ~0u;
        }
        const int qi = act ? i : 0;
        const u32 q = ((u32)ql[qi >> 1] >> ((qi & 1) * 4)) & 15u;
        int hd[S], hu[S], fu[S];
        fm_chain_fetch<G, S>(Hp, (int)l + dl, w2, hd);
        fm_chain_fetch<G, S>(Hp, (int)l + dl + 1, w2, hu);
        fm_chain_fetch<G, S>(Fp, (int)l + dl + 1, w2, fu);
        int H[S], F[S], x[S];
        u32 fl[S];
        bool ok[S];
#pragma unroll
        for (int s = 0; s < S; s++) {
            const int k = (int)l + 64 * s, col = i + c + k;
            ok[s] = act && k <= w2 && col >= J.clo && col < J.chi;
            u32 t;
            if (J.wn) {
                const int cc = ok[s] ? col - J.wlo : 0;
                t = ((u32)tl[cc >> 2] >> ((cc & 3) * 2)) & 3u;
            } else {
                t = ok[s] ? text_symbol(text, (u64)(J.tbase + col)) : 0u;
            }
            const bool eq = q == t;                            // q = 4 (not a base) equals no text code
            fl[s] = (hd[s] > 0 ? FM_EXT_SRC_DIAG : FM_EXT_SRC_START) | (eq ? 0u : FM_EXT_MISMATCH);
            H[s] = (hd[s] > 0 ? hd[s] : 0) + (eq ? sa : -sb);
            const int fo = hu[s] - goe, fe = fu[s] - se;
            F[s] = fo;
            if (fe > fo) { F[s] = fe; fl[s] |= FM_EXT_F_EXT; }
            x[s] = ok[s] ? (H[s] > F[s] ? H[s] : F[s]) + k * se : FM_EXT_NEG;
        }
        // exclusive prefix maximum of x over the band indices of the group
        int ex[S];
        {
            int v[S];
#pragma unroll
            for (int s = 0; s < S; s++) v[s] = x[s];
#pragma unroll
            for (int o = 1; o < G; o <<= 1) {
#pragma unroll
                for (int s = 0; s < S; s++) {
                    const int u = __shfl_up(v[s], o, G);
                    if ((int)l >= o && u > v[s]) v[s] = u;
                }
            }
#pragma unroll
            for (int s = 0; s < S; s++) {
                const int u = __shfl_up(v[s], 1, G);
                ex[s] = l ? u : FM_EXT_NEG;
            }
            if (S == 2) {
                const int tot = __shfl(v[0], G - 1, G);
                if (tot > ex[S - 1]) ex[S - 1] = tot;
            }
        }
        int E[S];
#pragma unroll
        for (int s = 0; s < S; s++) {
            const int k = (int)l + 64 * s;
            const int e = ex[s] - so - k * se;
            int h = H[s];
            if (e > h) { h = e; fl[s] = (fl[s] & ~3u) | FM_EXT_SRC_E; }
            if (F[s] > h) { h = F[s]; fl[s] = (fl[s] & ~3u) | FM_EXT_SRC_F; }
            H[s] = ok[s] ? h : FM_EXT_NEG; E[s] = ok[s] ? e : FM_EXT_NEG; F[s] = ok[s] ? F[s] : FM_EXT_NEG;
        }
        int hl[S], el[S];                                      // the finished left neighbour: did E continue its gap?
#pragma unroll
        for (int s = 0; s < S; s++) {
            const int a = __shfl_up(H[s], 1, G), b = __shfl_up(E[s], 1, G);
            hl[s] = l ? a : FM_EXT_NEG; el[s] = l ? b : FM_EXT_NEG;
        }
        if (S == 2) {
            const int a = __shfl(H[0], G - 1, G), b = __shfl(E[0], G - 1, G);
            if (!l) { hl[S - 1] = a; el[S - 1] = b; }
        }
#pragma unroll
        for (int s = 0; s < S; s++) {
            if (el[s] - se > hl[s] - goe) fl[s] |= FM_EXT_E_EXT;
            if (ok[s]) {
                ncell++;
                if (TRACE) fl_out[(size_t)r * (u32)(w2 + 1) + 64 * s] = (u8)fl[s];
                if (H[s] > bestS) { bestS = H[s]; bestI = i; bestK = (int)l + 64 * s; }
            }
            Hp[s] = H[s]; Fp[s] = F[s];
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

// Traceback, one lane per job, as k_fm_extend_trace: tr[4j ..] = qbeg, column of tbeg (signed: a chain may drift below
// column 0), edits, number of CIGAR ops; ops == NULL counts only.
__global__ __launch_bounds__(256) void k_fm_chain_trace(const FmChainJob *__restrict__ jobs,
                                                        const FmChainAnchor *__restrict__ anchors, u32 njobs, u32 w,
                                                        const u8 *__restrict__ flags, const u64 *__restrict__ best,
                                                        const u64 *__restrict__ cig_off, u32 *__restrict__ ops,
                                                        u32 *__restrict__ tr) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    const u64 key = best[j];
    u32 qbeg = 0, cbeg = 0, edits = 0, nops = 0;
    if (key >> 32) {
        const FmChainJob J = jobs[j];
        const FmChainAnchor *A = anchors + J.aoff;
        const int w2 = 2 * (int)w;
        int i = 65535 - (int)((key >> 8) & 0xFFFFu);
        u32 a = J.na - 1;                                      // the anchor in effect at row i
        while (a > 0 && A[a].q > (u32)i) a--;
        int col = i + A[a].dc + 127 - (int)(key & 0xFFu);
        u64 wp = ops ? cig_off[j + 1] : 0;
        const u64 wp0 = ops ? cig_off[j] : 0;
        u32 state = 0, cur = 3, len = 0;                      // state 0: in H, 1: in E (deletion), 2: in F (insertion)
        bool done = false;
        for (u64 guard = 4ull * J.m + 8ull * (w + 1) * J.na + 16; guard && !done; guard--) {
            if (i < (int)J.i0 || i >= (int)(J.i0 + J.nrows)) break;
            while (a > 0 && A[a].q > (u32)i) a--;
            const int k = col - i - A[a].dc;
            if (k < 0 || k > w2) break;
            const u32 fl = flags[J.flag_off + (size_t)(i - (int)J.i0) * (u32)(w2 + 1) + (u32)k];
            u32 op;
            if (state == 0) {
                const u32 src = fl & 3u;
                if (src == FM_EXT_SRC_E) { state = 1; continue; }
                if (src == FM_EXT_SRC_F) { state = 2; continue; }
                op = 0; edits += (fl >> 4) & 1u;
                qbeg = (u32)i; cbeg = (u32)col;
                if (src == FM_EXT_SRC_START) done = true; else { i--; col--; }
            } else if (state == 1) {
                op = 2; edits++;
                state = (fl & FM_EXT_E_EXT) ? 1u : 0u;
                col--;                                         // (i, t - 1)
            } else {
                op = 1; edits++;
                state = (fl & FM_EXT_F_EXT) ? 2u : 0u;
                i--;                                           // (i - 1, t)
            }
            if (op == cur) { len++; continue; }
            if (len) { nops++; if (ops && wp > wp0) ops[--wp] = (len << 4) | cur; }
            cur = op; len = 1;
        }
        if (len) { nops++; if (ops && wp > wp0) ops[--wp] = (len << 4) | cur; }
    }
    tr[4 * j] = qbeg; tr[4 * j + 1] = cbeg; tr[4 * j + 2] = edits; tr[4 * j + 3] = nops;
}
