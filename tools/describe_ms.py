"""dev tool (GPU box): psx_describe against psx_extract on one 1080p VLFeat-mode frame, one context, event timers
(psx_stage_times; medians over N runs after 5 warm-up runs, interleaved A/B/C in one process on one box).
  A  psx_extract                        [pyramid, extrema, orientation + scan, descriptors]
  B  psx_describe(REUSE_PYRAMID)        [-, keypoint injection, orientation + adopt + scan, descriptors] on A's own keypoints
  C  psx_describe(0)                    [pyramid, keypoint injection, orientation + adopt + scan, descriptors]
  D  B with the detector's orientations given (the orientation kernel's result is overwritten)
usage: python tools/describe_ms.py [runs] [seed] [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from popsift_amd import capi
from popsift_amd.synth import synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
ctx = capi.Context(capi.default_config(octaves=5, sift_mode=2))
ctx.upload(synth(1920, 1080, seed))
ctx.extract()
F, D = ctx.download()
lpos = np.concatenate([ctx.dump_iext(o)["lpos"] for o in range(ctx.num_octaves)])
recs = np.zeros(len(F), capi.KEYPOINT_DTYPE)
for name in ("xpos", "ypos", "sigma"):
    recs[name] = F[name]
recs["octave"], recs["lpos"] = F["debug_octave"], lpos
given = recs.copy()
given["num_ori"], given["orientation"] = F["num_ori"], F["orientation"]
ctx.enable_timers(True)
rows = {k: [] for k in "ABCD"}
for i in range(n + 5):
    for k in "ABCD":
        if k == "A":
            ctx.extract()
        else:
            ctx.set_keypoints(given if k == "D" else recs)
            ctx.sync()                                  # the list's copy is not part of the describe call's stages
            ctx.describe(reuse_pyramid=(k != "C"))
        ctx.sync()
        if i >= 5:
            rows[k].append(ctx.stage_times())
        if k == "A":
            ctx.counts()
med = {k: [round(float(v), 4) for v in np.median(np.array(rows[k]), axis=0)] for k in rows}
res = {"frame": "1920x1080 synth seed %d, VLFeat mode, 5 octaves" % seed, "keypoints": int(len(F)), "descriptors": int(len(D)),
       "runs": n, "stage_ms_median": {"extract": med["A"], "describe_reuse_pyramid": med["B"], "describe_with_pyramid": med["C"],
                                      "describe_reuse_pyramid_given_orientations": med["D"]},
       "orientation_plus_descriptors_ms": {"extract": round(med["A"][2] + med["A"][3], 4),
                                           "describe_reuse_pyramid": round(sum(med["B"][1:]), 4),
                                           "describe_reuse_pyramid_given_orientations": round(sum(med["D"][1:]), 4)},
       "whole_ms": {"extract": round(sum(med["A"]), 4), "describe_with_pyramid": round(sum(med["C"]), 4)},
       "extrema_stage_ms_vs_injection_ms": [med["A"][1], med["B"][1]]}
print(json.dumps(res))
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(res, f, indent=1)
