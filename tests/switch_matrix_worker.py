"""Worker of tests/test_gpu_switch_matrix.py: one process = one setting of the environment switches (a context reads them at
psx_create, the matcher once per thread when it binds its scratch to a device).  argv: a JSON file
{"family": .., "frames": [names]} or {"family": "match", "sequence": name}, and an output directory.

Frames (tests/switch_matrix_cases.FRAMES): writes <frame>.npz with the octave dimensions, the initial extrema of every
octave, the oriented extrema, the features and descriptors (those of the zero-copy export for the family
"orient_desc_export") and, for the family "pyramid", the digests of every Gaussian plane
(tests/full_size_cases.plane_digests).  Matcher: writes match.npz with the (best, second, accept) records and the distances
of every call of the sequence, and prints what match_f32_run derives from this device's CU count for each -- another device
shows another expectation.  Every C-ABI call that fails raises: the
process ends there with a non-zero status and starts nothing else on the device.  Prints one JSON line of what was done."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from popsift_amd import capi                    # noqa: E402
from tests import full_size_cases as fc         # noqa: E402
from tests import switch_matrix_cases as sc     # noqa: E402


def device_cus():
    info = capi.device_info(0)
    print("device 0: %s, %d compute units" % (info["name"], info["compute_units"]), flush=True)
    return info["compute_units"]


def run_frame(frame, family, out_dir):
    w, h, seed, kw = sc.FRAMES[frame]
    img = sc.image(frame)
    t0 = time.perf_counter()
    ctx = capi.Context(capi.default_config(**kw))
    export = family == "orient_desc_export"
    if export:
        pf = np.zeros(40000 * capi.FEATURE_DTYPE.itemsize, dtype=np.uint8)     # registered (pinned + mapped) by psx_attach_export
        pd = np.zeros(80000 * 128, dtype=np.float32)
        ctx.attach_export(pf, pd)
    ctx.upload(img)
    ctx.extract()
    ne, no = ctx.counts()                           # raises when a bounded device-side wait of k_pyramid_flow gave up
    t1 = time.perf_counter()
    nn = ctx.num_octaves
    rec = dict(num_octaves=np.int32(nn), num_levels=np.int32(ctx.num_levels), counts=np.array([ne, no], np.int32),
               dims=np.array([ctx.octave_dims(o) for o in range(nn)], np.int32).reshape(-1, 2))
    for o in range(nn):
        if family == "pyramid":
            for l in range(ctx.num_levels):
                sha, rows, cols = fc.plane_digests(ctx.dump_plane(capi.PLANE_GAUSS, o, l))
                rec["sha_%d_%d" % (o, l)] = np.array(sha)
                rec["rows_%d_%d" % (o, l)] = rows
                rec["cols_%d_%d" % (o, l)] = cols
        ie = ctx.dump_iext(o)
        for f in ("xpos", "ypos", "lpos"):
            rec["iext_%s_%d" % (f, o)] = np.ascontiguousarray(ie[f])
    rec["extrema"] = ctx.dump_extrema()
    if export:
        fb, db = ctx.exported()
        fb, db = fb.copy(), db.copy()
        ctx.attach_export(None, None)
    else:
        fb, db = ctx.download()
    ctx.close()
    rec["features"] = fb
    rec["descriptors"] = db
    np.savez(os.path.join(out_dir, frame + ".npz"), **rec)
    print("%s: %d keypoints, %d descriptors, create + upload + extract %.3f s" % (frame, ne, no, t1 - t0), flush=True)


def run_match(sequence, out_dir, cus):
    wgs = int(os.environ.get("POPSIFT_MATCH_WGS_PER_CU", "0"))
    rounds = int(os.environ.get("POPSIFT_MATCH_ROUNDS", "1"))
    mfma = not os.environ.get("POPSIFT_MATCH_MFMA", "1").startswith("0")
    rec = {}
    for i, (label, kind, l_len, r_len) in enumerate(sc.MATCH_SEQUENCES[sequence]):
        # unset: the runtime's occupancy answer for the prefilter kernel, 3 workgroups per CU on gfx950
        plan = sc.match_plan(l_len, r_len, cus, wgs if wgs > 0 else 3, rounds, mfma)
        print("call %d (%s, %s) %d x %d on %d CUs%s: expecting %s" % (i, label, kind, l_len, r_len, cus,
              "" if wgs > 0 else " (3 workgroups per CU assumed)", json.dumps(plan)), flush=True)
        l, r = sc.match_sets(kind, l_len, r_len)
        t0 = time.perf_counter()
        mm, dd = capi.match(l, r)
        print("call %d: psx_match with its transfers %.3f s" % (i, time.perf_counter() - t0), flush=True)
        rec["match_%d" % i] = mm
        rec["dist_%d" % i] = dd
    np.savez(os.path.join(out_dir, "match.npz"), **rec)


def main(spec_path, out_dir):
    spec = json.load(open(spec_path))
    cus = device_cus()
    if spec["family"] == "match":
        run_match(spec["sequence"], out_dir, cus)
        print(json.dumps([spec["sequence"]]))
        return
    for frame in spec["frames"]:
        run_frame(frame, spec["family"], out_dir)
    print(json.dumps(list(spec["frames"])))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
