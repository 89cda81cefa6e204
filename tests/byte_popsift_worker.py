"""Worker of tests/test_gpu_byte_popsift.py (a fresh process per environment: POPSIFT_EXPORT and POPSIFT_PINNED_LIMIT_MB
are read once per process).  python -m tests.byte_popsift_worker OUT.npz FRAMES OUTSTANDING W H: the same frames through
PopSift in float mode and in byte mode (VLFeat mode, 4 octaves), `OUTSTANDING` jobs in flight; saves every frame's
records and descriptors of both modes and the pinned pool's counters after each pass."""
import sys

import numpy as np

from popsift_amd import capi
from popsift_amd.synth import synth


def run(frames, outstanding, byte_descriptors):
    """two passes over the frames through ONE PopSift (a steady stream): the results of the second pass, and the pool's
    allocations after the first pass (warm-up), after the second, and its bytes in use after close()"""
    ps = capi.PopSift(capi.default_config(octaves=4, sift_mode=2, norm_multi=9), byte_descriptors=byte_descriptors)
    allocs = []
    for _ in range(2):
        out, jobs = [], []
        for img in frames:
            jobs.append(ps.enqueue(img))
            if len(jobs) >= outstanding:
                out.append(ps.get(jobs.pop(0)))
        while jobs:
            out.append(ps.get(jobs.pop(0)))
        allocs.append(capi.pool_stats(0)["allocs"])
    ps.close()
    return out, np.array(allocs + [capi.pool_stats(0)["in_use"]], np.int64)


def main():
    path, n, outstanding, w, h = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    frames = [synth(w, h, 900 + (i % 6)) for i in range(n)]
    save = {}
    for name, b in (("f32", False), ("u8", True)):
        res, pool = run(frames, outstanding, b)
        for i, (f, d) in enumerate(res):
            save["%s_feat_%d" % (name, i)] = f
            save["%s_desc_%d" % (name, i)] = d
        save["%s_pool" % name] = pool
    np.savez(path, **save)


if __name__ == "__main__":
    main()
