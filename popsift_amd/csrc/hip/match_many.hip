// match_many.hip -- one byte descriptor set against many in one call: psx_match_pairs_many_u8 (+ _dev), psx_match_many_plan.
//
// psx_match_pairs_u8 (match.hip) is two directed passes of the exact i8-MFMA matcher and a join: per call a fixed launch
// sequence, one synchronisation and one count read-back.  An image has 2k-4k descriptors: at that size the MFMA work is
// microseconds and the call is launch latency and the synchronisation, paid again for every right set.  The byte matcher
// already walks the right side in chunks of <= 512 rows that leave a per-left top-2 key each, merged in index order; the
// (distance, index) order is total, so the result does not depend on where the chunks are cut.  "One left set against K
// right sets" is that dataflow driven by tables in which no chunk crosses a set boundary (match_many_plan.h):
// The matcher's device pieces -- row norm, padding, tile walk, chunk merge, accept -- are those of k_match_u8, stated once in
// match_u8_core.h; the kernels here only say where the operands live:
//   k_u8_norms_many        |x - 128|^2 of every row of all K + 1 sets, each set padded to u8_pad(len)
//   k_match_u8_many        the walk of k_match_u8; its outer rows come from a block table, its inner rows from a chunk
//                          table.  Forward: blocks of L x chunks of the K right sets; backward (PSX_PAIRS_MUTUAL only): blocks
//                          of the K right sets x chunks of L -- the same kernel on the other pair of tables
//   k_match_u8_many_merge  per (outer row, inner set) the chunks of that set in index order: the directed result
//                          (match_scratch.h) the join reads -- K results per left row forward, one per right row backward
//   k_many_count / k_many_scan / k_many_write   the join of match.hip, segmented (match_many_join.h, shared with the
//                          guided one-to-many call): the rule of match_rule.h (psx_match_keep) per (set, left) counted per
//                          workgroup, a scan of the totals, one 16-byte store per survivor
// Launches per call, whatever K is: the table copy, the norms, 2 per direction, 3 for the join -- 8 kernels with the
// cross-check, 6 without; one stream synchronisation.  The per-chunk partials are the one buffer that grows with
// (chunks x outer rows): above MANY_PARTIAL_BUDGET the sets are processed in groups of whole sets, each group its own
// match + merge on the same stream (2 more launches per extra group, no synchronisation).
#include "psx_internal.h"
#include "match_join.h"
#include "match_many_join.h"
#include "match_many_plan.h"
#include "match_scratch.h"
#include "match_u8_core.h"

#include <climits>
#include <cstring>
#include <vector>

namespace {

constexpr size_t MANY_PARTIAL_BUDGET = (size_t)256 << 20;    // bytes of per-chunk partials one group of sets may take

// one entry per set: 0 .. K-1 the right sets, K the left set
struct ManySet {
    const unsigned char* desc;   // the set's descriptors
    int len;                     // rows
    int noff;                    // first entry of its norms in the norm array (a multiple of U8_TILE: 16-byte aligned)
    int roff;                    // its first row among the rows of its side (the right sets: prefix sum of the lengths; L: 0)
    int c0, c1;                  // its chunks in the chunk table
    int pad;
};
static_assert(sizeof(ManySet) == 32, "two 16-byte scalar loads per entry");

// which part of the tables a launch walks, and where its rows lie in the partials
struct ManyPass {
    int nblocks, block_base;     // outer blocks [block_base, block_base + nblocks)
    int chunk_base;              // the partials' first chunk
    int row_base, outer_rows;    // the partials hold outer rows [row_base, row_base + outer_rows) of the outer side
};

// grid: every block of both sides, 256 threads, 8 lanes per descriptor.  A set's norms are written up to u8_pad(len), the
// padding with zeros: the set's last block writes it.
__global__ __launch_bounds__(256) void k_u8_norms_many(const ManySet* __restrict__ sets, const int2* __restrict__ blocks,
                                                       int* __restrict__ norms)
{
    const int2 blk = blocks[blockIdx.x];
    const ManySet s = sets[blk.x];
    const int end = blk.y + PSX_MANY_BLOCK >= s.len ? (int)u8_pad(s.len) : blk.y + PSX_MANY_BLOCK;
    const int q = threadIdx.x & 7;
    for (int d = blk.y + (threadIdx.x >> 3); d < end; d += 32) {
        const int ss = u8_row_norm(s.desc, s.len, d, q);
        if (q == 0) norms[s.noff + d] = ss;
    }
}

// grid nblocks x (chunks of the launch), 256 threads; workgroup (ob, ch) = (blockIdx.x % nblocks, blockIdx.x / nblocks).
// k_match_u8 with both sides taken from tables: wave w owns outer rows [row0 + 64 w, + 64) of ITS block's set and walks
// rows [r0, r1) of ITS chunk's set (match_u8_core.h).  The two table entries are read at wave-uniform addresses (scalar
// loads).  Row reads are clamped to the set's own last row, idle outer columns repeat the last row of their own set, keys
// of rows past the chunk's end are U8_NONE: nothing of a neighbouring set is ever ranked.
// partial[ch * outer_rows + (row among the launch's outer rows)] = (smallest, second smallest key).
__global__ __launch_bounds__(256) void k_match_u8_many(const ManySet* __restrict__ sets, const int4* __restrict__ chunks,
                                                       const int2* __restrict__ blocks, const int* __restrict__ norms,
                                                       ManyPass ps, uint2* __restrict__ partial)
{
    const int ob = (int)(blockIdx.x % (unsigned)ps.nblocks), ch = (int)(blockIdx.x / (unsigned)ps.nblocks);
    const int2 blk = blocks[ps.block_base + ob];
    const int4 chk = chunks[ps.chunk_base + ch];
    const ManySet os = sets[blk.x], is = sets[chk.x];
    U8Wave w;
    u8_load_cols(w, os.desc, norms + os.noff, os.len, blk.y + (threadIdx.x >> 6) * 64);
    u8_walk(w, is.desc, norms + is.noff, is.len, chk.y, chk.z);
    u8_store_keys(w, os.len, partial + (size_t)ch * ps.outer_rows + (size_t)(os.roff - ps.row_base));
}

// grid nblocks x ngroups, 256 threads: one thread per (outer row of block ob, inner set group_base + g).  The set's chunks
// in table order = index order, merged as k_match_u8_merge merges them (u8_merge_chunk).  The result goes where the join
// expects the directed result of (outer set, inner set): at out + out_stride * (inner set) + 5 * (outer set's first row).
// out_stride = 5 l_len forward (K results per left row), 0 backward (the one inner set is L).
__global__ __launch_bounds__(256) void k_match_u8_many_merge(const ManySet* __restrict__ sets, const int4* __restrict__ chunks,
                                                             const int2* __restrict__ blocks, ManyPass ps, int group_base,
                                                             size_t out_stride, const uint2* __restrict__ partial, int* __restrict__ out)
{
    const int ob = (int)(blockIdx.x % (unsigned)ps.nblocks), g = group_base + (int)(blockIdx.x / (unsigned)ps.nblocks);
    const int2 blk = blocks[ps.block_base + ob];
    const ManySet os = sets[blk.x], is = sets[g];
    const int row = blk.y + (int)threadIdx.x;
    if (row >= os.len) return;
    const size_t prow = (size_t)(os.roff - ps.row_base) + row;
    U8Best t;
    for (int c = is.c0; c < is.c1; c++)
        u8_merge_chunk(t, partial[(size_t)(c - ps.chunk_base) * ps.outer_rows + prow], chunks[c].y);
    psx_directed_store<int>(out + out_stride * (size_t)g + 5 * (size_t)os.roff, os.len, (size_t)row, t.i1, t.i2, u8_accept(t.d1, t.d2), t.d1, t.d2);
}

// a run of whole sets whose partials fit the budget: what one match + merge pair of launches takes
struct ManyGroup { int block0, nblocks, chunk0, nchunks, set0, nsets, row0, rows; };

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// host_pairs or d_pairs (the other is NULL; both NULL with capacity 0)
int match_pairs_many(int device, const unsigned char* d_left, int l_len, const unsigned char* const* d_rights, const int* r_lens,
                     int n_sets, const psx_match_opts* opts, void* host_pairs, void* d_pairs, int capacity, int* set_counts, int* count)
{
    if (!psx_pairs_args_ok(l_len, 0, opts, host_pairs ? host_pairs : d_pairs, capacity, count) || (l_len > 0 && !d_left) ||
        n_sets < 0 || (n_sets > 0 && (!d_rights || !r_lens || !set_counts)) || !psx_many_sets_ok(l_len, r_lens, n_sets))
        return PSX_ERR_INVALID;
    long long r_total = 0;
    for (int k = 0; k < n_sets; k++) {
        if (r_lens[k] > 0 && !d_rights[k]) return PSX_ERR_INVALID;
        r_total += r_lens[k];
    }
    if (l_len == 0 || r_total == 0) {
        for (int k = 0; k < n_sets; k++) set_counts[k] = 0;
        *count = 0;
        return PSX_OK;
    }
    const bool mutual = (opts->flags & PSX_PAIRS_MUTUAL) != 0;
    const int K = n_sets;

    // ---- the plan: blocks and chunks of both sides (match_many_plan.h), on the host ----
    thread_local std::vector<psx_many_block> rblk, lblk;
    thread_local std::vector<psx_many_chunk> rchk, lchk;
    const long long BR = psx_many_blocks(r_lens, K, nullptr, 0), BL = psx_many_blocks(&l_len, 1, nullptr, 0);
    const long long CR = psx_many_chunks(r_lens, K, BL, nullptr, 0);
    const long long CL = mutual ? psx_many_chunks(&l_len, 1, BR, nullptr, 0) : 0;
    const long long nb = BL, ntot = (long long)K * nb;               // the join's workgroups
    if (ntot + 1 > INT_MAX) return PSX_ERR_NOMEM;
    rblk.resize((size_t)BR); lblk.resize((size_t)BL); rchk.resize((size_t)CR); lchk.resize((size_t)CL);
    psx_many_blocks(r_lens, K, rblk.data(), BR);
    psx_many_blocks(&l_len, 1, lblk.data(), BL);
    psx_many_chunks(r_lens, K, BL, rchk.data(), CR);
    if (mutual) psx_many_chunks(&l_len, 1, BR, lchk.data(), CL);

    // groups of whole sets within the partials' budget: forward over the right sets' chunks, backward over their blocks
    std::vector<ManyGroup> fgroups, bgroups;
    size_t partial_bytes = 0;
    for (long long c = 0; c < CR;) {
        ManyGroup g = {(int)BR, (int)BL, (int)c, 0, rchk[(size_t)c].set, 0, 0, l_len};
        while (c < CR) {
            long long e = c;                                         // the end of the next set's chunks
            while (e < CR && rchk[(size_t)e].set == rchk[(size_t)c].set) e++;
            if (g.nchunks > 0 && sizeof(uint2) * (size_t)(e - g.chunk0) * l_len > MANY_PARTIAL_BUDGET) break;
            g.nchunks = (int)(e - g.chunk0);
            g.nsets = rchk[(size_t)e - 1].set + 1 - g.set0;
            c = e;
        }
        if ((long long)g.nblocks * g.nchunks > INT_MAX || (long long)g.nblocks * g.nsets > INT_MAX) return PSX_ERR_NOMEM;
        const size_t b = sizeof(uint2) * (size_t)g.nchunks * l_len;
        if (b > partial_bytes) partial_bytes = b;
        fgroups.push_back(g);
    }
    std::vector<long long> roff((size_t)K + 1, 0);
    for (int k = 0; k < K; k++) roff[(size_t)k + 1] = roff[(size_t)k] + r_lens[k];
    if (mutual)
        for (long long b = 0; b < BR;) {
            const int s0 = rblk[(size_t)b].set;
            ManyGroup g = {(int)b, 0, (int)CR, (int)CL, s0, 0, (int)roff[(size_t)s0], 0};
            while (b < BR) {
                long long e = b;
                while (e < BR && rblk[(size_t)e].set == rblk[(size_t)b].set) e++;
                const int s = rblk[(size_t)b].set;
                const long long rows = roff[(size_t)s + 1] - g.row0;
                if (g.nblocks > 0 && sizeof(uint2) * (size_t)CL * (size_t)rows > MANY_PARTIAL_BUDGET) break;
                g.nblocks = (int)(e - g.block0);
                g.nsets = s + 1 - g.set0;
                g.rows = (int)rows;
                b = e;
            }
            if ((long long)g.nblocks * g.nchunks > INT_MAX) return PSX_ERR_NOMEM;
            const size_t bytes = sizeof(uint2) * (size_t)g.nchunks * (size_t)g.rows;
            if (bytes > partial_bytes) partial_bytes = bytes;
            bgroups.push_back(g);
        }

    // ---- sizes: the norms of all sets, the tables, the results ----
    long long npad = 0;
    for (int k = 0; k < K; k++) npad += r_lens[k] > 0 ? u8_pad(r_lens[k]) : 0;
    const long long l_noff = npad;
    npad += u8_pad(l_len);
    if (npad > INT_MAX) return PSX_ERR_NOMEM;
    const size_t sets_b = pad16(sizeof(ManySet) * ((size_t)K + 1));
    const size_t chunks_b = pad16(sizeof(int4) * (size_t)(CR + CL));
    const size_t blocks_b = pad16(sizeof(int2) * (size_t)(BR + BL));
    const size_t blob_b = sets_b + chunks_b + blocks_b;
    const long long all_pairs = (long long)K * l_len;                 // at most l_len pairs per set exist
    const size_t nrec = host_pairs ? (size_t)(capacity < all_pairs ? capacity : all_pairs) : 0;
    const size_t off_counts = 16, off_rec = off_counts + pad16(sizeof(int) * (size_t)K), off_blob = off_rec + 16 * nrec;

    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    // every buffer before the first launch: nothing is reallocated under queued work
    if (!sc.need(MS_MANY_TABLES, blob_b) || !sc.need(MS_MANY_NORMS, sizeof(int) * (size_t)npad) || !sc.need(MS_MANY_PARTIAL, partial_bytes) ||
        !sc.need(MS_MANY_FWD, sizeof(int) * 5 * (size_t)all_pairs) || (mutual && !sc.need(MS_MANY_BWD, sizeof(int) * 5 * (size_t)r_total)) ||
        !sc.need(MS_MANY_TOT, sizeof(int) * (2 * (size_t)ntot + 1)) || !sc.need_pinned(off_blob + blob_b))
        return PSX_ERR_NOMEM;
    void* dev_pin = nullptr;
    if (hipHostGetDevicePointer(&dev_pin, sc.hpin, 0) != hipSuccess || dev_pin == nullptr) return PSX_ERR_HIP;
    char* hp = static_cast<char*>(sc.hpin);

    // ---- the tables, written into the pinned staging buffer and copied on the stream ----
    {
        ManySet* hs = reinterpret_cast<ManySet*>(hp + off_blob);
        int4* hc = reinterpret_cast<int4*>(hp + off_blob + sets_b);
        int2* hb = reinterpret_cast<int2*>(hp + off_blob + sets_b + chunks_b);
        long long noff = 0;
        for (int k = 0; k < K; k++) {
            hs[k] = ManySet{d_rights[k], r_lens[k], (int)noff, (int)roff[(size_t)k], 0, 0, 0};
            noff += r_lens[k] > 0 ? u8_pad(r_lens[k]) : 0;
        }
        hs[K] = ManySet{d_left, l_len, (int)l_noff, 0, (int)CR, (int)(CR + CL), 0};
        for (long long c = 0; c < CR; c++) {
            const psx_many_chunk& q = rchk[(size_t)c];
            hc[c] = make_int4(q.set, q.r0, q.r1, 0);
            if (hs[q.set].c1 == 0) hs[q.set].c0 = (int)c;            // a set's chunks are contiguous: first and last + 1
            hs[q.set].c1 = (int)c + 1;
        }
        for (long long c = 0; c < CL; c++) hc[CR + c] = make_int4(K, lchk[(size_t)c].r0, lchk[(size_t)c].r1, 0);
        for (long long b = 0; b < BR; b++) hb[b] = make_int2(rblk[(size_t)b].set, rblk[(size_t)b].row0);
        for (long long b = 0; b < BL; b++) hb[BR + b] = make_int2(K, lblk[(size_t)b].row0);
    }
    int* h_total = reinterpret_cast<int*>(hp);
    *h_total = -1;
    const ManySet* d_sets = static_cast<const ManySet*>(sc.buf[MS_MANY_TABLES]);
    const int4* d_chunks = reinterpret_cast<const int4*>(static_cast<const char*>(sc.buf[MS_MANY_TABLES]) + sets_b);
    const int2* d_blocks = reinterpret_cast<const int2*>(static_cast<const char*>(sc.buf[MS_MANY_TABLES]) + sets_b + chunks_b);
    int* d_norms = static_cast<int*>(sc.buf[MS_MANY_NORMS]);
    uint2* d_partial = static_cast<uint2*>(sc.buf[MS_MANY_PARTIAL]);
    int* d_fwd = static_cast<int*>(sc.buf[MS_MANY_FWD]);
    int* d_bwd = mutual ? static_cast<int*>(sc.buf[MS_MANY_BWD]) : nullptr;
    int* d_tot = static_cast<int*>(sc.buf[MS_MANY_TOT]);
    int* d_total = static_cast<int*>(dev_pin);
    int* d_counts = reinterpret_cast<int*>(static_cast<char*>(dev_pin) + off_counts);
    // the kernel's capacity for the host form is the staging buffer's (nrec <= capacity)
    int4* out = host_pairs ? reinterpret_cast<int4*>(static_cast<char*>(dev_pin) + off_rec) : static_cast<int4*>(d_pairs);
    const int cap = host_pairs ? (int)nrec : capacity;
    hipStream_t st = sc.stream;

    if (hipMemcpyAsync(sc.buf[MS_MANY_TABLES], hp + off_blob, blob_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_u8_norms_many, dim3((unsigned)(BR + BL)), dim3(256), 0, st, d_sets, d_blocks, d_norms);
    for (const ManyGroup& g : fgroups) {
        const ManyPass ps = {g.nblocks, g.block0, g.chunk0, g.row0, g.rows};
        hipLaunchKernelGGL(k_match_u8_many, dim3((unsigned)g.nblocks * (unsigned)g.nchunks), dim3(256), 0, st, d_sets, d_chunks, d_blocks,
                           d_norms, ps, d_partial);
        hipLaunchKernelGGL(k_match_u8_many_merge, dim3((unsigned)g.nblocks * (unsigned)g.nsets), dim3(256), 0, st, d_sets, d_chunks,
                           d_blocks, ps, g.set0, 5 * (size_t)l_len, d_partial, d_fwd);
    }
    for (const ManyGroup& g : bgroups) {
        const ManyPass ps = {g.nblocks, g.block0, g.chunk0, g.row0, g.rows};
        hipLaunchKernelGGL(k_match_u8_many, dim3((unsigned)g.nblocks * (unsigned)g.nchunks), dim3(256), 0, st, d_sets, d_chunks, d_blocks,
                           d_norms, ps, d_partial);
        hipLaunchKernelGGL(k_match_u8_many_merge, dim3((unsigned)g.nblocks), dim3(256), 0, st, d_sets, d_chunks, d_blocks, ps, K,
                           (size_t)0, d_partial, d_bwd);
    }
    psx_many_join_queue<int>(st, d_sets, d_fwd, l_len, d_bwd, (int)nb, (int)ntot, opts->ratio, mutual, d_tot, out, cap, d_counts, d_total);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
    const int n = *h_total;
    if (n < 0 || n > all_pairs) return PSX_ERR_HIP;
    memcpy(set_counts, hp + off_counts, sizeof(int) * (size_t)K);
    if (host_pairs && n > 0 && nrec > 0) memcpy(host_pairs, hp + off_rec, 16 * ((size_t)n < nrec ? (size_t)n : nrec));
    *count = n;
    return PSX_OK;
}

} // namespace

extern "C" int psx_match_pairs_many_u8(int device, const unsigned char* d_left, int l_len,
                                       const unsigned char* const* d_rights, const int* r_lens, int n_sets,
                                       const psx_match_opts* opts, psx_match_pair_u8* host_pairs, int capacity,
                                       int* set_counts, int* count)
{
    return match_pairs_many(device, d_left, l_len, d_rights, r_lens, n_sets, opts, host_pairs, nullptr, capacity, set_counts, count);
}

extern "C" int psx_match_pairs_many_u8_dev(int device, const unsigned char* d_left, int l_len,
                                           const unsigned char* const* d_rights, const int* r_lens, int n_sets,
                                           const psx_match_opts* opts, psx_match_pair_u8* d_pairs, int capacity,
                                           int* set_counts, int* count)
{
    return match_pairs_many(device, d_left, l_len, d_rights, r_lens, n_sets, opts, nullptr, d_pairs, capacity, set_counts, count);
}

extern "C" int psx_match_many_plan(int l_len, const int* r_lens, int n_sets, int backward,
                                   psx_many_chunk* chunks, int chunk_capacity, int* chunk_count,
                                   psx_many_block* blocks, int block_capacity, int* block_count)
{
    return psx_many_plan_host(l_len, r_lens, n_sets, backward, chunks, chunk_capacity, chunk_count, blocks, block_capacity, block_count);
}
