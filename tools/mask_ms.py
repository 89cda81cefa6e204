"""dev tool (GPU box): what a detection mask buys and what a per-job host mask costs, on the 1080p VLFeat bench frame.
  1. one context, device-resident input: single-frame wall time (extract + counts, median of N after 5 warm-up runs) and
     the event-timed stages (psx_stage_times, a second pass with the timers on) unmasked and with the masks `half`,
     `disc` and `zeros` (tests/mask_cases.py), interleaved in one process on one box;
  2. PopSift path: frames per second over the same frames without a mask and with a per-job host mask (`disc`): the
     extra 2 MB deep copy + upload per 1080p job.
usage: python tools/mask_ms.py [runs] [popsift_frames] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from popsift_amd import capi
from popsift_amd.synth import synth
from tests.mask_cases import make_mask

n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
nframes = int(sys.argv[2]) if len(sys.argv) > 2 else 400
W, H, KW = 1920, 1080, dict(octaves=5, sift_mode=2)
img = synth(W, H, 1000)
masks = {"none": None, "half": make_mask("half", W, H), "disc": make_mask("disc", W, H), "zeros": make_mask("zeros", W, H)}

ctx = capi.Context(capi.default_config(**KW))
t_img = torch.from_numpy(img).cuda()
torch.cuda.synchronize()
ctx.set_input_tensor(t_img)
wall = {k: [] for k in masks}
stages = {k: [] for k in masks}
counts = {}
for timed in (False, True):
    ctx.enable_timers(timed)
    for i in range(n + 5):
        for k, m in masks.items():
            ctx.set_mask(m)
            ctx.sync()                                   # the mask's copy is not part of the frame
            t0 = time.perf_counter()
            ctx.extract()
            counts[k] = ctx.counts()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= 5:
                (stages[k].append(ctx.stage_times()) if timed else wall[k].append(dt))
ctx.close()
res = {"frame": "1920x1080 synth seed 1000, VLFeat mode, 5 octaves, device-resident input", "runs": n,
       "features_descriptors": {k: list(v) for k, v in counts.items()},
       "single_frame_ms_median": {k: round(float(np.median(v)), 4) for k, v in wall.items()},
       "stage_ms_median [pyramid, extrema, orientation+scan, descriptors]":
           {k: [round(float(x), 4) for x in np.median(np.array(v), axis=0)] for k, v in stages.items()}}

frames = [synth(W, H, 1000 + i) for i in range(8)]
fps = {}
for rep in range(2):
    for tag, m in (("no_mask", None), ("per_job_host_mask_disc", masks["disc"])):
        ps = capi.PopSift(capi.default_config(**KW))
        for j in [ps.enqueue(frames[i % 8], mask=m) for i in range(32)]:
            ps.get_counts(j)
        t0 = time.perf_counter()
        for j in [ps.enqueue(frames[i % 8], mask=m) for i in range(nframes)]:
            ps.get_counts(j)
        fps.setdefault(tag, []).append(round(nframes / (time.perf_counter() - t0), 1))
        ps.close()
res["popsift_frames_per_second (two runs each, %d frames)" % nframes] = fps
print(json.dumps(res))
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(res, f, indent=1)
