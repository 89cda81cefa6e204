// match_scratch.h -- what the matcher's translation units share (match.hip, match_guided.hip): the per-thread scratch and
// the runner of the pair join.  Internal to the HIP library.
#pragma once

#include "psx_internal.h"

// Scratch of one calling thread: a private non-blocking stream (no null-stream launch, so nothing else on
// the device is synchronised) and buffers that only ever grow.  Freed when the thread exits.
struct MatchScratch {
    // 0-9: psx_match, 10-12: psx_match_u8; the pair search: 13 the backward direction's results of psx_match_pairs,
    // 14 those of psx_match_pairs_u8, 15 the join's per-workgroup totals; guided matching (match_guided.hip): 16 the forward
    // direction's results, 17 the backward direction's, 18 the left side's lines for the backward direction; the homography
    // RANSAC (ransac.hip): 19 the uploaded pair records, 20 the packed correspondences, 21 the hypotheses' models, 22 their
    // counts, 23 the state block, 24 the compaction's per-workgroup totals; the one-to-many byte pair search
    // (match_many.hip): 25 the set / chunk / block tables, 26 the norms of all sets, 27 the per-chunk partials, 28 the forward
    // direction's results of all sets, 29 the backward direction's, 30 the join's per-workgroup totals and their offsets
    static constexpr int NBUF = 31;
    int device = -1;
    hipStream_t stream = nullptr;
    void* buf[NBUF] = {};
    size_t cap[NBUF] = {};
    void* hpin = nullptr;                // pinned staging of the results: a DMA into pageable caller memory goes through the
    size_t hpin_cap = 0;                 // runtime's own bounce buffers, ~0.5 ms per call on this stack
    bool tidy = false;                   // the prefilter's counters are zero (left so by the previous call's last kernel)
    PsxTuning tune;                      // the POPSIFT_MATCH_* switches and the CU count of `device`: taken in bind()
    int mfma_per_cu = 0;                 // workgroups of the prefilter kernel resident per CU on `device` (0: not asked yet)
    void release()
    {
        if (device < 0) return;
        int cur = -1;                                        // the caller's current device is left as it was
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        (void)hipSetDevice(device);
        for (int i = 0; i < NBUF; i++) { (void)hipFree(buf[i]); buf[i] = nullptr; cap[i] = 0; }
        tidy = false;
        if (hpin) (void)hipHostFree(hpin);
        hpin = nullptr; hpin_cap = 0;
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr; device = -1;
        if (cur >= 0) (void)hipSetDevice(cur);
    }
    // the scratch of `device` (a call for another device releases the previous one's first)
    bool bind(int dev)
    {
        if (device == dev) return true;
        release();
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return false;
        device = dev;
        tune = psx_tuning_from_env();
        if (hipDeviceGetAttribute(&tune.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || tune.cus <= 0) tune.cus = 256;
        mfma_per_cu = 0;
        return true;
    }
    bool need_pinned(size_t bytes)
    {
        if (bytes <= hpin_cap && hpin) return true;
        if (hpin) (void)hipHostFree(hpin);
        hpin = nullptr; hpin_cap = 0;
        if (hipHostMalloc(&hpin, bytes, hipHostMallocDefault) != hipSuccess) return false;
        hpin_cap = bytes;
        return true;
    }
    bool need(int i, size_t bytes)
    {
        if (bytes <= cap[i] && buf[i]) return true;
        (void)hipFree(buf[i]); buf[i] = nullptr; cap[i] = 0;
        tidy = false;
        if (hipMalloc(&buf[i], bytes) != hipSuccess) return false;
        cap[i] = bytes;
        return true;
    }
    // Thread exit.  For the main thread that is process teardown, where the HIP runtime may already be gone: ask it
    // first (a finalised runtime answers with an error) and then leave the buffers to the process exit.
    ~MatchScratch() { int n = 0; if (device >= 0 && hipGetDeviceCount(&n) == hipSuccess && n > 0) release(); }
};

// the calling thread's scratch (one object per thread, whichever translation unit asks: psx_match_release frees it)
MatchScratch& psx_match_scratch();

// Queues the join (k_pairs_count / k_pairs_write, match.hip) behind the directed passes already queued on sc.stream and
// finishes the call.  d_fwd / d_bwd: a directed pass' device results -- 3 len ints (best, second, accept), then 2 len
// distances (float / int); d_bwd is read only with PSX_PAIRS_MUTUAL.  host_pairs or d_pairs (the other is NULL; both
// NULL with capacity 0).  One synchronisation.
int psx_pairs_finish_f32(MatchScratch& sc, const int* d_fwd, int l_len, const int* d_bwd, const psx_match_opts* opts,
                         void* host_pairs, void* d_pairs, int capacity, int* count);
int psx_pairs_finish_u8(MatchScratch& sc, const int* d_fwd, int l_len, const int* d_bwd, const psx_match_opts* opts,
                        void* host_pairs, void* d_pairs, int capacity, int* count);
