// match_many_f32_plan.h -- how psx_match_pairs_many (match_many_f32.hip, include/popsift_hip.h) lays out one call: which
// of its two paths runs, how each side is cut, and how the sets are grouped under the scratch budget.
//
// Plain C++14, no HIP: match_many_f32.hip plans with psx_many_f32_build, psx_match_many_f32_plan reports what it
// decides, and a stand-alone program can include the header alone (tests/cpp/match_many_f32_plan_san.cpp).
//
// The blocks of a side (256 outer rows of one set) and the chunks of the exact scan (whole tiles of 32 rows, at most 512,
// never across a set boundary) are those of match_many_plan.h.  The prefilter's chunks are longer -- every (outer row,
// chunk) seeds its running maxima afresh and owns 2 x 32 candidate slots, so fewer, longer chunks cost fewer candidates and
// less memory -- whole staged blocks of 64 rows, at least PSX_MANYF_PRE_MIN rows unless the set is shorter, and no more of
// them than one round of resident workgroups takes (psx_manyf_pre_chunks).
// One buffer grows with (chunks x outer rows): the scan's per-chunk top-2 (16 bytes each) or the prefilter's candidate
// segments (2 x (32 x 4 + 4) bytes each).  Above PSX_MANYF_BUDGET the call walks WHOLE SETS in groups on one stream:
// forward a group is a run of right sets (its chunks x all of L), backward a run of right sets' blocks (x all chunks of L).
#pragma once

#include "match_many_plan.h"
#include "popsift_hip.h"

#include <vector>

constexpr long long PSX_MANYF_BUDGET = 256LL << 20;   // bytes one group's growing buffer may take (match_many.hip's figure)
constexpr int PSX_MANYF_MIN_L = 256;                  // the prefilter runs from this many left rows ...
constexpr int PSX_MANYF_MIN_R = 4096;                 // ... and this many right rows IN ALL SETS on (match.hip: 256 and 2 * MF_SEED)
constexpr int PSX_MANYF_SCAN_UNIT = 16;               // bytes per (outer row, chunk): the scan's top-2
constexpr int PSX_MANYF_SEGCAP = 32;                  // candidate slots per (outer row, chunk, half wave)
constexpr int PSX_MANYF_PRE_UNIT = 2 * (PSX_MANYF_SEGCAP * 4 + 4);   // the prefilter's: two segments and their counts
constexpr int PSX_MANYF_PRE_STEP = 64;                // rows per staged block of the prefilter kernel
constexpr int PSX_MANYF_PRE_MIN = 512;                // a prefilter chunk is not cut shorter than this
constexpr int PSX_MANYF_PRE_MAX = 4096;               // ... nor longer than this: a segment's 32 slots fill with the chunk's length
constexpr int PSX_MANYF_PRE_WGS = 768;                // (block, chunk) workgroups a prefilter pass aims at: 256 CUs x 3 resident

struct psx_manyf_group { int block0, nblocks, chunk0, nchunks, set0, nsets, row0, rows; };

struct psx_manyf_tables {
    int path = 0;                                     // 0: no pair can exist, 1: scan, 2: prefilter
    std::vector<psx_many_block> rblk, lblk;           // outer blocks of the right sets / of L
    std::vector<psx_many_chunk> rchk, lchk;           // inner chunks of the right sets / of L (lchk: with the cross-check only)
    std::vector<psx_manyf_group> fgroups, bgroups;
    long long scratch_bytes = 0;                      // the largest group's growing buffer
    int launches = 0;                                 // kernels queued when the flag stays down
};

// the rule: the single call's two thresholds on the call's totals, one decision for both directions
inline int psx_manyf_path(int l_len, const int* r_lens, int n_sets, bool mfma_enabled)
{
    long long rows = 0;
    for (int k = 0; k < n_sets; k++) rows += r_lens[k];
    if (l_len == 0 || rows == 0) return 0;
    return (mfma_enabled && l_len >= PSX_MANYF_MIN_L && rows >= PSX_MANYF_MIN_R) ? 2 : 1;
}

// The prefilter's chunks of a side.  A pass should fit ONE round of resident workgroups (a few workgroups past it cost the
// time of a second round), and every chunk start costs candidates: so the chunk length is the SMALLEST number of whole
// staged blocks, at least PSX_MANYF_PRE_MIN and at most PSX_MANYF_PRE_MAX, with which all sets together give at most
// floor(PSX_MANYF_PRE_WGS / outer_blocks) chunks -- or one chunk per set where the sets alone are more than that.  Every set is then cut into
// equal pieces of whole staged blocks, as psx_many_chunks cuts the scan's.
inline long long psx_manyf_pre_chunks(const int* lens, int n, long long outer_blocks, psx_many_chunk* out, long long cap)
{
    long long longest = 0, nonempty = 0;
    for (int s = 0; s < n; s++) { if (lens[s] > longest) longest = lens[s]; if (lens[s] > 0) nonempty++; }
    if (outer_blocks < 1) outer_blocks = 1;
    long long want = PSX_MANYF_PRE_WGS / outer_blocks;
    if (want < nonempty) want = nonempty;
    if (want < 1) want = 1;
    // the chunk count falls as the length grows: bisect on the length in staged blocks
    long long lo = PSX_MANYF_PRE_MIN / PSX_MANYF_PRE_STEP, hi = (longest + PSX_MANYF_PRE_STEP - 1) / PSX_MANYF_PRE_STEP;
    if (hi > PSX_MANYF_PRE_MAX / PSX_MANYF_PRE_STEP) hi = PSX_MANYF_PRE_MAX / PSX_MANYF_PRE_STEP;
    if (hi < lo) hi = lo;
    while (lo < hi) {
        const long long mid = (lo + hi) / 2, len = mid * PSX_MANYF_PRE_STEP;
        long long chunks = 0;
        for (int s = 0; s < n; s++) chunks += (lens[s] + len - 1) / len;
        if (chunks <= want) hi = mid; else lo = mid + 1;
    }
    const long long target = lo * PSX_MANYF_PRE_STEP;
    long long c = 0;
    for (int s = 0; s < n; s++) {
        const long long len = lens[s];
        if (len <= 0) continue;
        const long long pieces = (len + target - 1) / target;
        long long step = (len + pieces - 1) / pieces;
        step = ((step + PSX_MANYF_PRE_STEP - 1) / PSX_MANYF_PRE_STEP) * PSX_MANYF_PRE_STEP;
        for (long long r0 = 0; r0 < len; r0 += step, c++)
            if (out != nullptr && c < cap) {
                out[c].set = s; out[c].r0 = (int)r0; out[c].r1 = (int)(r0 + step < len ? r0 + step : len);
            }
    }
    return c;
}

// Tables and groups of one call on `path` (1 or 2).  false: a count does not fit an int (the caller answers NOMEM).
inline bool psx_many_f32_build(int l_len, const int* r_lens, int n_sets, bool mutual, int path, psx_manyf_tables& t)
{
    t = psx_manyf_tables();
    t.path = path;
    if (path == 0) return true;
    const long long LIM = 2147483647LL;
    const long long unit = path == 2 ? PSX_MANYF_PRE_UNIT : PSX_MANYF_SCAN_UNIT;
    const long long BR = psx_many_blocks(r_lens, n_sets, nullptr, 0), BL = psx_many_blocks(&l_len, 1, nullptr, 0);
    t.rblk.resize((size_t)BR); t.lblk.resize((size_t)BL);
    psx_many_blocks(r_lens, n_sets, t.rblk.data(), BR);
    psx_many_blocks(&l_len, 1, t.lblk.data(), BL);
    const long long CR = path == 2 ? psx_manyf_pre_chunks(r_lens, n_sets, BL, nullptr, 0) : psx_many_chunks(r_lens, n_sets, BL, nullptr, 0);
    const long long CL = !mutual ? 0 : path == 2 ? psx_manyf_pre_chunks(&l_len, 1, BR, nullptr, 0) : psx_many_chunks(&l_len, 1, BR, nullptr, 0);
    if (BR + BL > LIM || CR + CL > LIM) return false;
    t.rchk.resize((size_t)CR); t.lchk.resize((size_t)CL);
    if (path == 2) psx_manyf_pre_chunks(r_lens, n_sets, BL, t.rchk.data(), CR); else psx_many_chunks(r_lens, n_sets, BL, t.rchk.data(), CR);
    if (mutual) { if (path == 2) psx_manyf_pre_chunks(&l_len, 1, BR, t.lchk.data(), CL); else psx_many_chunks(&l_len, 1, BR, t.lchk.data(), CL); }

    // forward: runs of whole right sets whose chunks x l_len fit the budget
    for (long long c = 0; c < CR;) {
        psx_manyf_group g = {(int)BR, (int)BL, (int)c, 0, t.rchk[(size_t)c].set, 0, 0, l_len};
        while (c < CR) {
            long long e = c;                                         // the end of the next set's chunks
            while (e < CR && t.rchk[(size_t)e].set == t.rchk[(size_t)c].set) e++;
            if (g.nchunks > 0 && unit * (e - g.chunk0) * l_len > PSX_MANYF_BUDGET) break;
            g.nchunks = (int)(e - g.chunk0);
            g.nsets = t.rchk[(size_t)e - 1].set + 1 - g.set0;
            c = e;
        }
        // the grids: (block, chunk) workgroups; the exact evaluation's 64 workgroups per (block, set)
        if ((long long)g.nblocks * g.nchunks > LIM || (long long)g.nblocks * 64 * g.nsets > LIM) return false;
        if (path == 2 && 2LL * PSX_MANYF_SEGCAP * g.nchunks * (g.nblocks * 256LL) > LIM) return false;      // a candidate slot's index is an int
        const long long b = unit * g.nchunks * l_len;
        if (b > t.scratch_bytes) t.scratch_bytes = b;
        t.fgroups.push_back(g);
    }
    // backward: runs of whole right sets whose rows x the chunks of L fit the budget
    if (mutual) {
        std::vector<long long> roff((size_t)n_sets + 1, 0);
        for (int k = 0; k < n_sets; k++) roff[(size_t)k + 1] = roff[(size_t)k] + r_lens[k];
        for (long long b = 0; b < BR;) {
            const int s0 = t.rblk[(size_t)b].set;
            psx_manyf_group g = {(int)b, 0, (int)CR, (int)CL, s0, 0, (int)roff[(size_t)s0], 0};
            while (b < BR) {
                long long e = b;
                while (e < BR && t.rblk[(size_t)e].set == t.rblk[(size_t)b].set) e++;
                const int s = t.rblk[(size_t)b].set;
                const long long rows = roff[(size_t)s + 1] - g.row0;
                if (g.nblocks > 0 && unit * CL * rows > PSX_MANYF_BUDGET) break;
                g.nblocks = (int)(e - g.block0);
                g.nsets = s + 1 - g.set0;
                g.rows = (int)rows;
                b = e;
            }
            if ((long long)g.nblocks * g.nchunks > LIM || (long long)g.nblocks * 64 > LIM) return false;
            if (path == 2 && 2LL * PSX_MANYF_SEGCAP * g.nchunks * (g.rows + 256LL) > LIM) return false;
            const long long bytes = unit * g.nchunks * g.rows;
            if (bytes > t.scratch_bytes) t.scratch_bytes = bytes;
            t.bgroups.push_back(g);
        }
    }
    // scan: the permutation, (partial, merge) per group, the join's three; prefilter: norms, conversion, (prefilter, exact
    // evaluation) per group, the join's three
    t.launches = (path == 2 ? 2 : 1) + 2 * (int)(t.fgroups.size() + t.bgroups.size()) + 3;
    return true;
}

// psx_match_many_f32_plan (include/popsift_hip.h)
inline int psx_many_f32_plan_host(int l_len, const int* r_lens, int n_sets, int flags, int mfma_enabled, psx_many_f32_plan* out)
{
    if (!psx_many_sets_ok(l_len, r_lens, n_sets) || out == nullptr || (flags & ~PSX_PAIRS_MUTUAL) != 0 ||
        (mfma_enabled != 0 && mfma_enabled != 1))
        return PSX_ERR_INVALID;
    psx_manyf_tables t;
    if (!psx_many_f32_build(l_len, r_lens, n_sets, (flags & PSX_PAIRS_MUTUAL) != 0, psx_manyf_path(l_len, r_lens, n_sets, mfma_enabled != 0), t))
        return PSX_ERR_NOMEM;
    out->path = t.path;
    out->fwd_groups = (int)t.fgroups.size();
    out->bwd_groups = (int)t.bgroups.size();
    out->launches = t.launches;
    out->scratch_bytes = t.scratch_bytes;
    return PSX_OK;
}
