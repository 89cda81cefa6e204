"""Worker of tests/test_gpu_mask.py (a fresh process: PopSift owns worker threads and pinned pools).
python -m tests.mask_popsift_worker OUT.npz: three images x (no mask, mask A, mask B) through one capi.Context each --
the single-context reference -- and 48 jobs through one capi.PopSift, alternating masked and unmasked, from 4 caller
threads (two rounds); the pinned pool's counters after a warm-up that holds every result and at the end; one masked
job through a byte-descriptor PopSift."""
import sys
import threading

import numpy as np

from popsift_amd import capi
from popsift_amd.synth import synth
from tests.mask_cases import make_mask

KW = dict(octaves=4, sift_mode=2, norm_multi=9)
W, H = 640, 480
NJOBS, NTHREADS = 48, 4


def job_spec(i):
    """(image index, mask name or None) of job i: masked and unmasked alternate, two different masks"""
    return i % 3, (None, "checker1", None, "disc")[i % 4]


def main():
    path = sys.argv[1]
    save = {}
    imgs = [synth(W, H, 40 + k) for k in range(3)]
    masks = {None: None, "checker1": make_mask("checker1", W, H), "disc": make_mask("disc", W, H)}
    ctx = capi.Context(capi.default_config(**KW))
    for k, img in enumerate(imgs):
        for name, m in masks.items():
            ctx.upload(img)
            ctx.set_mask(m)
            ctx.extract()
            save["ctx_feat_%d_%s" % (k, name)], save["ctx_desc_%d_%s" % (k, name)] = ctx.download()
    ctx.close()

    ps = capi.PopSift(capi.default_config(**KW))
    results = [None] * NJOBS
    errors = []

    def caller(t, first, last):
        try:
            jobs = []
            for i in range(first + t, last, NTHREADS):
                k, name = job_spec(i)
                jobs.append((i, ps.enqueue(imgs[k], mask=masks[name])))
            for i, j in jobs:
                results[i] = ps.get(j)
        except Exception as e:                      # reported by the parent test
            errors.append("%d: %r" % (t, e))

    def round_of(first, last):
        threads = [threading.Thread(target=caller, args=(t, first, last)) for t in range(NTHREADS)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()

    # Warm-up to the pool's high-water mark.  How many buffers are alive at once in a round depends on how the 8
    # workers and the 4 callers interleave: up to 48 images + 24 masks, and on top of them anything from a handful to
    # workers + callers result buffers.  A plain round therefore does not bring the pool to a state the next round
    # cannot exceed.  This warm-up does: TWICE the jobs of a round, all of them in the queue before the first result is
    # taken (every worker takes one and gets its export window; 96 images + 48 masks alive together, more small buffers
    # than a round can ever want), and every result is HELD until the last one is in (two descriptor buffers of every
    # job's size alive together, more than a round can have in flight of any size).
    hostlib = capi.host_lib()
    held, hold_lock = [], threading.Lock()

    def warm_caller(t):
        try:
            jobs = [ps.enqueue(imgs[job_spec(i)[0]], mask=masks[job_spec(i)[1]]) for i in range(t, 2 * NJOBS, NTHREADS)]
            for j in jobs:
                f = hostlib.popsift_c_get(j)
                if not f:
                    raise capi.PopSiftError(hostlib.popsift_c_last_error().decode())
                with hold_lock:
                    held.append(f)
        except Exception as e:
            errors.append("warm-up %d: %r" % (t, e))

    threads = [threading.Thread(target=warm_caller, args=(t,)) for t in range(NTHREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for f in held:
        hostlib.popsift_c_free(f)
    warm = capi.pool_stats()
    round_of(0, NJOBS)
    round_of(0, NJOBS)
    end = capi.pool_stats()
    ps.close()
    save["errors"] = np.array(errors, dtype="U200")
    save["pool_warm"] = np.array([warm["allocs"], warm["frees"]], np.int64)
    save["pool_end"] = np.array([end["allocs"], end["frees"]], np.int64)
    for i, r in enumerate(results):
        if r is not None:
            save["ps_feat_%d" % i], save["ps_desc_%d" % i] = r

    pb = capi.PopSift(capi.default_config(**KW), byte_descriptors=True)
    save["bytes_feat"], save["bytes_desc"] = pb.get(pb.enqueue(imgs[0], mask=masks["disc"]))
    pb.close()
    np.savez(path, **save)


if __name__ == "__main__":
    main()
