// fm_kmer_kernels.h -- k-mer counts along reads and k-mer read correction.  The count of a k-mer is a backward search of
// k steps (fm_occ2); a prefix table of the row intervals of all q-mers lets a search start from the interval of its
// last q characters.  Profile: one lane per (read, position, strand); the two strands of a position sit in neighbouring
// lanes and are added with one shuffle.  Correction: per round the profile, one lane per read that lists the trials of
// its weak runs (fm_weak_trials, shared with the host export), one lane per (trial, base, strand) that counts the
// substituted k-mer, and one lane per read that applies the fixes.
// Single TU: included by debwt_hip.hip only, after fm_mem_kernels.h.
#pragma once
#include "common.h"
#include "fm_kernels.h"
#include "fm_search_kernels.h"
#include "fm_mem_kernels.h"

#define FM_KMER_MAX_Q 12u
#define FM_KMER_NOFIX 0xFFu

// counters of the k-mer kernels (u64 each)
enum { FM_KM_STEPS = 0, FM_KM_READS, FM_KM_WSTEPS, FM_KM_TSTART, FM_KM_TRIALS, FM_KM_FIXES, FM_KM_ACTIVE, FM_KM_KMERS, FM_KM_NCTR = 8 };

// Runs of weak k-mers (counts[j] < min_count) of one read and their trials, the definition of debwt_fm_weak_trials:
// emit(run_a, run_b, pos, window, kind) is called for each trial, runs ascending, left (kind 0) before right (kind 1).
// Returns the number of weak k-mers.
template <typename Emit>
__host__ __device__ inline u32 fm_weak_trials(const u32 *counts, u32 nk, u32 k, u32 min_count, Emit emit) {
    u32 weak = 0;
    for (u32 a = 0; a < nk;) {
        if (counts[a] >= min_count) { a++; continue; }
        u32 b = a;
        while (b + 1 < nk && counts[b + 1] < min_count) b++;
        const u32 len = b - a + 1;
        weak += len;
        if (a > 0 && (len >= k || b == nk - 1)) emit(a, b, a + k - 1, a, 0u);
        if (b < nk - 1 && (len >= k || a == 0)) emit(a, b, b, b, 1u);
        a = b + 1;
    }
    return weak;
}

// code of position x of the query string of a k-mer W = p[0 .. k): W itself (strand 0) or its reverse complement
// (strand 1); position sub of W (none: sub >= k) reads as code subc instead of its byte
__device__ __forceinline__ u32 fm_kmer_code(const u8 *__restrict__ p, u32 k, u32 strand, u32 x, u32 sub, u32 subc) {
    const u32 w = strand ? k - 1 - x : x;
    const u32 c = w == sub ? subc : fm_code(p[w]);
    return (strand && c < 4) ? 3u - c : c;
}

// occ of the k-mer (0 when it holds a non-base): from the table entry of its last q characters when k >= q > 0, else
// from [0, n); one fm_occ2 per remaining character while the interval is not empty
__device__ __forceinline__ u64 fm_kmer_occ(const VIndex &V, const u64 *__restrict__ table, u32 q, const u8 *__restrict__ p,
                                           u32 k, u32 strand, u32 sub, u32 subc, u64 &steps, u64 &reads, u64 &tstart) {
    u64 lo = 0, hi = V.n;
    u32 x = k;
    if (q && k >= q) {
        u64 idx = 0;
        u32 bad = 0;
        for (u32 t = k - q; t < k; t++) {
            const u32 c = fm_kmer_code(p, k, strand, t, sub, subc);
            bad |= c >> 2;
            idx = (idx << 2) | (c & 3u);
        }
        if (bad) return 0;
        lo = table[2 * idx]; hi = table[2 * idx + 1];
        x = k - q;
        tstart++;
    }
    while (x > 0 && lo < hi) {
        const u32 c = fm_kmer_code(p, k, strand, x - 1, sub, subc);
        if (c > 3) return 0;
        fm_mem_step(V, c, lo, hi, &lo, &hi, steps, reads);
        x--;
    }
    return hi > lo ? hi - lo : 0;
}

// the one place where a count is clamped to u32
__device__ __forceinline__ u32 fm_kmer_clamp(u64 cnt) { return cnt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)cnt; }

__device__ __forceinline__ void fm_kmer_counters(u64 steps, u64 reads, u64 tstart, bool counted, u64 *__restrict__ ctr) {
    const u64 wmax = fm_wave_max(steps), ws = fm_wave_sum(steps), wr = fm_wave_sum(reads), wt = fm_wave_sum(tstart);
    const u64 wk = (u64)__popcll(__ballot(counted));
    if (lane_id() == 0 && wk) {
        atomicAdd((unsigned long long *)&ctr[FM_KM_KMERS], (unsigned long long)wk);
        atomicAdd((unsigned long long *)&ctr[FM_KM_STEPS], (unsigned long long)ws);
        atomicAdd((unsigned long long *)&ctr[FM_KM_READS], (unsigned long long)wr);
        atomicAdd((unsigned long long *)&ctr[FM_KM_WSTEPS], (unsigned long long)(64 * wmax));
        atomicAdd((unsigned long long *)&ctr[FM_KM_TSTART], (unsigned long long)wt);
    }
}

// Prefix table, level by level in place: level l holds the intervals of all l-mers in table[0 .. 4^l) (first character
// the most significant digit).  The l-mer c w is entry c * 4^(l-1) + index(w) and follows from w's entry by one step, so
// lane i < 4^(l-1) reads entry i alone and writes entries i + c * 4^(l-1): no lane reads what another writes.  Level 0
// is the single entry [0, n), set by the host.  An empty interval stays [lo, lo) as k_fm_count leaves it.
__global__ __launch_bounds__(256) void k_fm_kmer_table_level(VIndex V, u64 *__restrict__ table, u64 prev) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= prev) return;
    const u64 lo = table[2 * i], hi = table[2 * i + 1];
    u64 ol[4] = {0, 0, 0, 0}, oh[4] = {0, 0, 0, 0};
    if (lo < hi) (void)fm_occ4(V, lo, hi, ol, oh);             // the four children from one read of the line(s)
#pragma unroll
    for (u32 c = 0; c < 4; c++) {
        u64 nl = lo, nh = hi;
        if (lo < hi) { nl = V.C[c] + ol[c]; nh = V.C[c] + oh[c]; if (nh < nl) nh = nl; }
        table[2 * (i + c * prev)] = nl; table[2 * (i + c * prev) + 1] = nh;
    }
}

// Profile of the batch's reads: lane g is position t = g / nstr of the batch (coff: np + 1 prefix sums of the reads'
// k-mer numbers, so read i owns [coff[i], coff[i + 1])) on strand g % nstr.  Consecutive lanes take consecutive positions
// of one read.  counts[t] = min(cnt, 2^32 - 1).  active (may be null): reads with active[i] == 0 are left alone.
__global__ __launch_bounds__(256) void k_fm_kmer_profile(VIndex V, const u64 *__restrict__ table, u32 q,
                                                         const u8 *__restrict__ chars, const u64 *__restrict__ offsets,
                                                         u64 base, const u64 *__restrict__ coff, u64 np, u64 nitems,
                                                         u32 k, u32 nstr, const u8 *__restrict__ active,
                                                         u32 *__restrict__ counts, u64 *__restrict__ ctr) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 strand = nstr == 2 ? (u32)(g & 1) : 0u;
    const u64 t = nstr == 2 ? g >> 1 : g;
    u64 steps = 0, reads = 0, tstart = 0, occ = 0;
    bool live = false;
    if (t < nitems) {                                          // no early return: the wave reductions below need all lanes
        const u64 i = upper_bound_dev<u64>(coff, 0, np + 1, t) - 1;
        live = !active || active[i];
        if (live) occ = fm_kmer_occ(V, table, q, chars + (offsets[i] - base) + (t - coff[i]), k, strand, k, 0, steps, reads, tstart);
    }
    if (nstr == 2) {                                           // the other strand of the same position: the neighbouring lane
        const u32 lo = (u32)__shfl_xor((int)(u32)occ, 1, 64), hi = (u32)__shfl_xor((int)(u32)(occ >> 32), 1, 64);
        occ += ((u64)hi << 32) | lo;
    }
    if (live && strand == 0) counts[t] = fm_kmer_clamp(occ);
    fm_kmer_counters(steps, reads, tstart, live && strand == 0, ctr);
}

// One lane per read of the batch: the weak k-mers of its profile and, unless count_only, its trials, written to slots
// coff[i] + i .. (a read of nk k-mers has at most nk + 1 trials: at most (nk + 1) / 2 runs of two).  trials: 2 u32 per
// slot, pos and window | kind << 31 in the read's coordinates; trun: the trial's run number.  info: 4 u32 per read
// {flags, fixes, weak_before, weak_after}; weak_after is the latest profile's number.
__global__ __launch_bounds__(256) void k_fm_correct_trials(const u64 *__restrict__ coff, u64 np, u32 k, u32 min_count,
                                                           const u32 *__restrict__ counts, const u8 *__restrict__ active,
                                                           u32 first, u32 count_only, u32 *__restrict__ trials,
                                                           u32 *__restrict__ trun, u32 *__restrict__ ntrials,
                                                           u32 *__restrict__ info, u64 *__restrict__ ctr) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np || !active[i]) return;
    const u64 c0 = coff[i];
    const u32 nk = (u32)(coff[i + 1] - c0);
    const u64 s0 = c0 + i;
    u32 nt = 0, run = 0, last_a = 0xFFFFFFFFu;
    const u32 weak = fm_weak_trials(counts + c0, nk, k, min_count, [&](u32 a, u32, u32 pos, u32 window, u32 kind) {
        if (count_only) return;
        if (a != last_a) { run++; last_a = a; }
        trials[2 * (s0 + nt)] = pos; trials[2 * (s0 + nt) + 1] = window | (kind << 31);
        trun[s0 + nt] = run;
        nt++;
    });
    if (first) info[4 * i + 2] = weak;
    info[4 * i + 3] = weak;
    if (!count_only) {
        ntrials[i] = nt;
        if (nt) atomicAdd((unsigned long long *)&ctr[FM_KM_TRIALS], (unsigned long long)nt);
    }
}

// One lane per (trial slot, base x, strand): the count of the trial's window with position pos replaced by x; the lanes
// of a slot are neighbours (4 * nstr of them), so the strands are added with one shuffle and the candidates of the four x
// are read from one ballot.  result[slot]: the single candidate's code, or FM_KMER_NOFIX.
__global__ __launch_bounds__(256) void k_fm_correct_eval(VIndex V, const u64 *__restrict__ table, u32 q,
                                                         const u8 *__restrict__ chars, const u64 *__restrict__ offsets,
                                                         u64 base, const u64 *__restrict__ coff, u64 np, u64 nslots,
                                                         u32 k, u32 nstr, u32 min_count, const u8 *__restrict__ active,
                                                         const u32 *__restrict__ trials, const u32 *__restrict__ ntrials,
                                                         u8 *__restrict__ result, u64 *__restrict__ ctr) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 strand = nstr == 2 ? (u32)(g & 1) : 0u;
    const u32 x = (u32)(nstr == 2 ? g >> 1 : g) & 3u;
    const u64 s = nstr == 2 ? g >> 3 : g >> 2;
    u64 steps = 0, reads = 0, tstart = 0, occ = 0;
    bool live = false, tested = false;
    if (s < nslots) {
        // slot s belongs to read i with coff[i] + i <= s < coff[i + 1] + i + 1
        u64 lo = 0, hi = np;
        while (hi - lo > 1) {
            const u64 mid = (lo + hi) >> 1;
            if (coff[mid] + mid <= s) lo = mid; else hi = mid;
        }
        const u64 i = lo, tr = s - (coff[i] + i);
        live = active[i] && tr < ntrials[i];
        if (live) {
            const u8 *r = chars + (offsets[i] - base);
            const u32 pos = trials[2 * s], window = trials[2 * s + 1] & 0x7FFFFFFFu;
            tested = fm_code(r[pos]) != x;
            if (tested) occ = fm_kmer_occ(V, table, q, r + window, k, strand, pos - window, x, steps, reads, tstart);
        }
    }
    if (nstr == 2) {
        const u32 lo = (u32)__shfl_xor((int)(u32)occ, 1, 64), hi = (u32)__shfl_xor((int)(u32)(occ >> 32), 1, 64);
        occ += ((u64)hi << 32) | lo;
    }
    const u64 cand = __ballot(tested && strand == 0 && fm_kmer_clamp(occ) >= min_count);
    const u32 per = 4 * nstr, l0 = lane_id() & ~(per - 1);
    if (live && lane_id() == l0) {
        u32 n = 0, which = 0;
        for (u32 b = 0; b < 4; b++)
            if ((cand >> (l0 + b * nstr)) & 1ull) { n++; which = b; }
        result[s] = n == 1 ? (u8)which : (u8)FM_KMER_NOFIX;
    }
    fm_kmer_counters(steps, reads, tstart, tested && strand == 0, ctr);
}

// One lane per read: per run the fix of its first successful trial, written into the read's bytes in upper case.  A
// read without a fix leaves the rounds (active[i] = 0); the others are counted in ctr[FM_KM_ACTIVE].
__global__ __launch_bounds__(256) void k_fm_correct_apply(u8 *__restrict__ chars, const u64 *__restrict__ offsets, u64 base,
                                                          const u64 *__restrict__ coff, u64 np,
                                                          const u32 *__restrict__ trials, const u32 *__restrict__ trun,
                                                          const u32 *__restrict__ ntrials, const u8 *__restrict__ result,
                                                          u8 *__restrict__ active, u32 *__restrict__ info,
                                                          u64 *__restrict__ ctr) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np || !active[i]) return;
    u8 *r = chars + (offsets[i] - base);
    const u64 s0 = coff[i] + i;
    const u32 nt = ntrials[i];
    u32 fixes = 0, fixed_run = 0;
    for (u32 t = 0; t < nt; t++) {
        const u32 x = result[s0 + t];
        if (x == FM_KMER_NOFIX || trun[s0 + t] == fixed_run) continue;
        r[trials[2 * (s0 + t)]] = (u8)("ACGT"[x]);
        fixed_run = trun[s0 + t];
        fixes++;
    }
    if (!fixes) { active[i] = 0; return; }
    info[4 * i + 1] += fixes;
    atomicAdd((unsigned long long *)&ctr[FM_KM_FIXES], (unsigned long long)fixes);
    atomicAdd((unsigned long long *)&ctr[FM_KM_ACTIVE], 1ull);
}
