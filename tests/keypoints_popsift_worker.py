"""Worker of tests/test_gpu_keypoints.py (a fresh process: PopSift owns worker threads and pinned pools).
python -m tests.keypoints_popsift_worker OUT.npz: for a byte and a float image, the detector's keypoints described
through capi.Context (explicit records, reversed order) and through capi.PopSift.enqueue(img, keypoints=...) -- three
jobs in flight, an empty list, a plain detector job, and (byte image) a PopSift with byte descriptors."""
import sys

import numpy as np

from popsift_amd import capi
from popsift_amd.synth import synth, synth_float

KW = dict(octaves=4, sift_mode=2, norm_multi=9)


def main():
    path = sys.argv[1]
    save = {}
    for tag, img in (("u8", synth(640, 480, 31)), ("f32", synth_float(480, 360, 32))):
        ctx = capi.Context(capi.default_config(**KW))
        ctx.upload(img)
        ctx.extract()
        F, D = ctx.download()
        save[tag + "_ctx_det_feat"], save[tag + "_ctx_det_desc"] = F, D
        lpos = np.concatenate([ctx.dump_iext(o)["lpos"] for o in range(ctx.num_octaves)])
        recs = np.zeros(len(F), capi.KEYPOINT_DTYPE)
        for name in ("xpos", "ypos", "sigma"):
            recs[name] = F[name]
        recs["octave"], recs["lpos"] = F["debug_octave"], lpos
        recs = recs[::-1].copy()
        ctx.set_keypoints(recs)
        ctx.describe()
        save[tag + "_ctx_feat"], save[tag + "_ctx_desc"] = ctx.download()
        save[tag + "_ctx_src"] = ctx.keypoint_map()
        ctx.close()

        ps = capi.PopSift(capi.default_config(**KW), float_images=(tag == "f32"))
        jobs = [ps.enqueue(img, keypoints=recs) for _ in range(3)]
        j_empty = ps.enqueue(img, keypoints=recs[:0])
        j_det = ps.enqueue(img)
        for k, j in enumerate(jobs):
            save["%s_ps_feat_%d" % (tag, k)], save["%s_ps_desc_%d" % (tag, k)], save["%s_ps_src_%d" % (tag, k)] = ps.get(j, with_sources=True)
        save[tag + "_ps_empty_feat"], _, save[tag + "_ps_empty_src"] = ps.get(j_empty, with_sources=True)
        save[tag + "_ps_det_feat"], save[tag + "_ps_det_desc"], save[tag + "_ps_det_src"] = ps.get(j_det, with_sources=True)
        ps.close()
        if tag == "u8":
            pb = capi.PopSift(capi.default_config(**KW), byte_descriptors=True)
            save["u8_ps_bytes_feat"], save["u8_ps_bytes_desc"] = pb.get(pb.enqueue(img, keypoints=recs))
            pb.close()
    np.savez(path, **save)


if __name__ == "__main__":
    main()
