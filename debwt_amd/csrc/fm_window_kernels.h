// fm_window_kernels.h -- affine-gap local alignment of (query, text window) jobs: the recurrence, the end cell and the
// traceback rule of fm_extend_kernels.h over ALL cells of a window [wbeg, wend) clipped to its record, without a band
// (mate rescue: there is no seed, only the insert-size range next to the partner).
// One wave works on one job.  The window (L columns, at most 16384) is cut into strips of 64 columns; lane l owns column
// c = 64 s + l of strip s and sweeps its anti-diagonals a = 0 .. m + (columns of the strip) - 2, computing row i = a - l
// at step a.  All inputs of a cell were produced one step earlier -- the upper neighbour (i - 1, c) is the lane's own
// register, the left neighbour (i, c - 1) the lower lane's by __shfl_up -- or two steps earlier: the diagonal
// predecessor (i - 1, c - 1) is the H that was shuffled in one step ago.  Lane 0 takes its left neighbour from the
// hand-over buffer in LDS: (H, E) of the last column of the strip before, 8 bytes per query row; lane 63 overwrites row i
// 63 steps after lane 0 read it, so one buffer serves reading and writing.  The query codes (4 bits each) and the
// window's text (2 bits each) are staged in LDS once per job.  Every lane keeps the first cell of its largest H in the
// contract's order (smaller row first); one packed-key reduction per job at the end.  With TRACE one byte of direction
// flags per cell goes to the job's slice of a scratch buffer, laid out by (strip, anti-diagonal, lane) so that a step
// stores 64 consecutive bytes; k_fm_window_trace walks it back with one lane per job.
// Flag scratch per job: ((strips - 1) (m + 63) + m + (columns of the last strip) - 1) x 64 bytes <= 64 (m + 63) strips.
// Single TU: included by debwt_hip.hip only, after fm_extend_kernels.h.
#pragma once
#include "common.h"
#include "fm_extend_kernels.h"

#define FM_WIN_MAX_LEN 4096u           // DEBWT_FM_WINDOW_MAX_QUERY: 12 bits of row in the key, 32 KiB of hand-over
#define FM_WIN_MAX_COLS 16384u         // DEBWT_FM_WINDOW_MAX_COLUMNS: 14 bits of column in the key

struct FmWinJob {
    u64 qoff;            // first byte of the pattern in the batch's characters
    u64 flag_off;        // first flag byte of the job (TRACE)
    u64 tbase;           // text position of window column 0 (the window clipped to the record)
    u32 m, strand;
    u32 ncol, nstrips;   // columns of the clipped window (>= 1) and their strips of 64
};

// LDS bytes of one job: hand-over, query codes, text codes (a multiple of 8)
__host__ __device__ __forceinline__ u32 fm_win_lds(u32 m, u32 ncol) {
    return (8u * m + ((m + 1) >> 1) + ((ncol + 3) >> 2) + 7u) & ~7u;
}

// best[j] = score << 32 | (4095 - i) << 14 | (16383 - c) of the job's best cell (c: window column): the largest H, then
// the smallest query index, then the smallest text position (0 in the high word: no positive cell).  cells[j]: cells
// computed.  Dynamic LDS: lds_per_job bytes for each of the blockDim.x / 64 jobs of a workgroup.
template <bool TRACE>
__global__ __launch_bounds__(256) void k_fm_window(const u64 *__restrict__ text, const u8 *__restrict__ chars,
                                                   const FmWinJob *__restrict__ jobs, u32 njobs, int sa, int sb, int so,
                                                   int se, u32 lds_per_job, u8 *__restrict__ flags,
                                                   u64 *__restrict__ best, u32 *__restrict__ cells) {
    extern __shared__ __attribute__((aligned(8))) u8 fm_win_lds_mem[];
    const u32 l = threadIdx.x & 63u, wi = threadIdx.x >> 6;
    const u64 j = (u64)blockIdx.x * (blockDim.x >> 6) + wi;
    FmWinJob J{};                                              // no job: m = 0, no strip
    if (j < njobs) J = jobs[j];
    const int m = (int)J.m;
    int2 *hand = (int2 *)(fm_win_lds_mem + (size_t)wi * lds_per_job);
    u8 *ql = (u8 *)(hand + J.m), *tl = ql + ((J.m + 1) >> 1);
    {
        const u8 *p = chars + J.qoff;
        for (u32 x = l; x < (J.m + 1) >> 1; x += 64) {
            const u32 c0 = fm_mem_code(p, J.m, J.strand, 2 * x);
            const u32 c1 = 2 * x + 1 < J.m ? fm_mem_code(p, J.m, J.strand, 2 * x + 1) : 4u;
            ql[x] = (u8)(c0 | (c1 << 4));
        }
        const u32 nb = J.m ? (J.ncol + 3) >> 2 : 0;
        for (u32 x = l; x < nb; x += 64) {
            u32 b = 0;
#pragma unroll
            for (u32 q = 0; q < 4; q++)
                if (4 * x + q < J.ncol) b |= text_symbol(text, J.tbase + 4 * x + q) << (2 * q);
            tl[x] = (u8)b;
        }
    }
    __syncthreads();
    const int goe = so + se;
    int bestS = 0, bestI = 0, bestC = 0;
    u32 ncell = 0;
    for (u32 s = 0; s < J.nstrips; s++) {
        const int c = (int)(64 * s + l);
        const bool colok = (u32)c < J.ncol;
        const int cc = colok ? c : 0;
        const u32 t = ((u32)tl[cc >> 2] >> ((cc & 3) * 2)) & 3u;
        const u32 scols = J.ncol - 64 * s < 64 ? J.ncol - 64 * s : 64;
        const u32 nst = J.m + scols - 1;
        const bool first = s == 0, hands = scols == 64 && s + 1 < J.nstrips;
        u8 *fl_out = flags + J.flag_off + (size_t)s * (J.m + 63) * 64 + l;
        int H = FM_EXT_NEG, E = FM_EXT_NEG, F = FM_EXT_NEG, hd = FM_EXT_NEG;
        int2 nx = first ? make_int2(FM_EXT_NEG, FM_EXT_NEG) : hand[0];     // (H, E) of (row a, last column before the strip)
        for (u32 a = 0; a < nst; a++) {
            const int i = (int)a - (int)l;
            const bool ok = colok && i >= 0 && i < m;
            const int qi = ok ? i : 0;
            const u32 q = ((u32)ql[qi >> 1] >> ((qi & 1) * 4)) & 15u;
            int hl = __shfl_up(H, 1, 64), el = __shfl_up(E, 1, 64);
            if (l == 0) { hl = nx.x; el = nx.y; }
            if (!first) nx = hand[a + 1 < J.m ? a + 1 : J.m - 1];         // the next step's; past the last row nothing uses it
            const u32 fl = fm_ext_cell(ok, q, t, hd, hl, el, H, F, sa, sb, goe, se, H, E, F);
            hd = hl;
            if (ok) {
                ncell++;
                if (TRACE) fl_out[(size_t)a * 64] = (u8)fl;
                if (H > bestS || (H == bestS && H > 0 && i < bestI)) { bestS = H; bestI = i; bestC = c; }
                if (hands && l == 63) hand[i] = make_int2(H, E);
            }
        }
    }
    u64 key = bestS > 0 ? ((u64)(u32)bestS << 32) | ((u64)(4095 - bestI) << 14) | (u64)(16383 - bestC) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u32 lo = (u32)__shfl_xor((int)(u32)key, o, 64), hi = (u32)__shfl_xor((int)(u32)(key >> 32), o, 64);
        const u64 v = ((u64)hi << 32) | lo;
        key = v > key ? v : key;
        ncell += (u32)__shfl_xor((int)ncell, o, 64);
    }
    if (l == 0 && j < njobs) { best[j] = key; cells[j] = ncell; }
}

// Traceback, one lane per job, from the best cell back to the cell whose H started the alignment.  tr[4j ..]: qbeg,
// window column of tbeg, edits (mismatch columns + gap bases), number of CIGAR ops.  ops == NULL: count only; otherwise
// the ops (len << 4 | op, M 0, I 1, D 2) are written from cig_off[j + 1] downwards, so that they read left to right.
__global__ __launch_bounds__(256) void k_fm_window_trace(const FmWinJob *__restrict__ jobs, u32 njobs,
                                                         const u8 *__restrict__ flags, const u64 *__restrict__ best,
                                                         const u64 *__restrict__ cig_off, u32 *__restrict__ ops,
                                                         u32 *__restrict__ tr) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    const u64 key = best[j];
    u32 qbeg = 0, cbeg = 0, edits = 0, nops = 0;
    if (key >> 32) {
        const FmWinJob J = jobs[j];
        int i = 4095 - (int)((key >> 14) & 0xFFFu), c = 16383 - (int)(key & 0x3FFFu);
        u64 wp = ops ? cig_off[j + 1] : 0;
        const u64 wp0 = ops ? cig_off[j] : 0;
        u32 state = 0, cur = 3, len = 0;                      // state 0: in H, 1: in E (deletion), 2: in F (insertion)
        bool done = false;
        for (u32 guard = 2 * (J.m + J.ncol) + 8; guard && !done; guard--) {    // columns + state changes of any path
            if (i < 0 || i >= (int)J.m || c < 0 || c >= (int)J.ncol) break;
            const u32 s = (u32)c >> 6, ln = (u32)c & 63u;
            const u32 fl = flags[J.flag_off + ((size_t)s * (J.m + 63) + (u32)i + ln) * 64 + ln];
            u32 op;
            if (state == 0) {
                const u32 src = fl & 3u;
                if (src == FM_EXT_SRC_E) { state = 1; continue; }
                if (src == FM_EXT_SRC_F) { state = 2; continue; }
                op = 0; edits += (fl >> 4) & 1u;
                qbeg = (u32)i; cbeg = (u32)c;
                if (src == FM_EXT_SRC_START) done = true; else { i--; c--; }
            } else if (state == 1) {
                op = 2; edits++;
                state = (fl & FM_EXT_E_EXT) ? 1u : 0u;
                c--;                                           // (i, t - 1)
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
