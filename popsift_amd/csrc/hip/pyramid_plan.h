// pyramid_plan.h -- the launches of one frame's pyramid and extrema scans as a flat list of steps (psx_step,
// include/popsift_hip.h), built once per frame size in psx_resize and issued by the one loop of psx_build_pyramid;
// psx_find_extrema issues the same list's scan steps when the scans did not go out with the pyramid.
//
// Host arithmetic only: a plan is a pure function of the octave sizes, the level count, the spans, the tuning and the
// number of resident workgroups, so psx_pyramid_plan hands it out without a device (tests/test_pyramid_plan_cpu.py).
// The level-0 launch of octave 0 is not a step: every schedule starts with it (the prologue of psx_build_pyramid).
//
// What the ints of a step mean, unused ones are 0:
//   PSX_STEP_BLUR      level b of octave a in one launch
//   PSX_STEP_BLUR2     levels (a, b) and (c, d) in one launch (k_blur2)
//   PSX_STEP_TILE      launch a of the tile schedule (k_blur_tile)
//   PSX_STEP_FLOW      the one-launch flow kernel (k_pyramid_flow)
//   PSX_STEP_SCAN      the extrema scan of octave a as a launch of its own
//   PSX_STEP_SCAN_SET  one batched scan of the n <= PSX_EXT_BATCH octaves a, b, c, d
#pragma once

#include <vector>

#include "psx_internal.h"

typedef std::vector<psx_step> PsxPlan;

inline bool psx_step_is_scan(const psx_step& s) { return s.kind == PSX_STEP_SCAN || s.kind == PSX_STEP_SCAN_SET; }

// first: PSX_PLAN_TILE -- the first octave on the tile kernel, ntile its launches; PSX_PLAN_FLOW -- the first octave of
// the flow kernel's work list (0 or 1); ignored otherwise
inline void psx_pyramid_steps(const PsxParams& P, const int* inc_span, const PsxTuning& tune, int resident_blocks, int schedule,
                              int first, int ntile, PsxPlan& out)
{
    const int L = P.L, D = L - 3;
    int deferred[PSX_MAX_OCTAVES], ndef = 0;
    out.clear();
    auto blur = [&](int o, int level) { out.push_back(psx_step{PSX_STEP_BLUR, 0, o, level, 0, 0}); };
    // A large octave's scan goes out at once (right behind its last level its planes are as cache-resident as they will
    // ever be); an octave whose tiles do not fill the chip (a few hundred tiles, a latency-bound launch) is deferred and
    // shares one launch with the others at the end of the plan.
    auto scan = [&](int o) {
        if (psx_extrema_tiles(P, o) >= resident_blocks) out.push_back(psx_step{PSX_STEP_SCAN, 0, o, 0, 0, 0});
        else deferred[ndef++] = o;
    };
    auto octave_by_levels = [&](int o) { for (int level = 1; level < L; level++) blur(o, level); };

    if (schedule == PSX_PLAN_FLOW) {
        // octave 0's levels by launches first when the work list starts at octave 1 (POPSIFT_FLOW=2), then every remaining
        // blur level of the frame in ONE launch with device-side dependencies, then the scans
        if (first > 0) octave_by_levels(0);
        out.push_back(psx_step{PSX_STEP_FLOW, 0, 0, 0, 0, 0});
        for (int o = 0; o < P.num_octaves; o++) scan(o);
    } else if (schedule == PSX_PLAN_TILE) {
        // octaves in front of `first`: one launch per level, the octave's scan right behind its last level; then the tile
        // launches (several levels of up to two octaves each); then the scans of the tiled octaves
        for (int o = 0; o < first; o++) { octave_by_levels(o); scan(o); }
        for (int q = 0; q < ntile; q++) out.push_back(psx_step{PSX_STEP_TILE, 0, q, 0, 0, 0});
        for (int o = first; o < P.num_octaves; o++) scan(o);
    } else {
        // Diagonal schedule.  Level l of octave o only needs level l-1 of the same octave, and level 0 of octave o+1
        // is written by the launch of level D = L-3 of octave o; so octave o+1 may start D launch slots after octave
        // o, and (o+1, l) then shares ONE launch with (o, l+D) -- if the two planes fit one round of resident
        // workgroups (4 per CU).  The small octaves, chains of ~5 us launches on their own, ride along with the octave
        // above.  Where the pair does not fit (octave 0 / 1 of a 1080p frame) the smaller plane would only queue behind
        // a full chip, run on the larger radius' kernel for nothing and push the larger octave's planes out of L2
        // between its own levels: there octave o+1 starts after octave o's last level.
        auto pair_ok = [&](int o, int o2, int span) {
            return tune.batch_octaves && psx_blur_pair_ok(tune, P.oct[o].w, P.oct[o].h, P.oct[o2].w, P.oct[o2].h, span, resident_blocks);
        };
        int t0[PSX_MAX_OCTAVES];                       // level l of octave o runs in launch slot t0[o] + l
        t0[0] = 0;
        for (int o = 0; o + 1 < P.num_octaves; o++) t0[o + 1] = t0[o] + (pair_ok(o, o + 1, inc_span[L - 1]) ? D : L - 1);
        const int T = t0[P.num_octaves - 1] + L - 1;
        for (int t = 1; t <= T; t++) {
            int jo[4], nj = 0;
            for (int o = 0; o < P.num_octaves && nj < 4; o++)
                if (t - t0[o] >= 1 && t - t0[o] <= L - 1) jo[nj++] = o;
            for (int q = 0; q < nj; q += 2) {
                const int o = jo[q], level = t - t0[o];
                if (q + 1 == nj) { blur(o, level); continue; }
                // one launch only when both fit into one round of resident workgroups: behind a launch that fills the
                // chip the second plane would just queue, and it would run on the larger radius' kernel for nothing
                const int o2 = jo[q + 1], level2 = t - t0[o2];
                if (pair_ok(o, o2, inc_span[level] > inc_span[level2] ? inc_span[level] : inc_span[level2]))
                    out.push_back(psx_step{PSX_STEP_BLUR2, 0, o, level, o2, level2});
                else { blur(o, level); blur(o2, level2); }
            }
            for (int q = 0; q < nj; q++) if (t - t0[jo[q]] == L - 1) scan(jo[q]);
        }
    }
    static_assert(PSX_EXT_BATCH == 4, "a psx_step names four octaves");
    for (int i = 0; i < ndef; i += PSX_EXT_BATCH) {
        int o[PSX_EXT_BATCH] = {0, 0, 0, 0};
        const int m = ndef - i < PSX_EXT_BATCH ? ndef - i : PSX_EXT_BATCH;
        for (int k = 0; k < m; k++) o[k] = deferred[i + k];
        out.push_back(psx_step{PSX_STEP_SCAN_SET, m, o[0], o[1], o[2], o[3]});
    }
}
