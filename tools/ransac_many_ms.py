"""dev tool (GPU box): what one batched verification call costs beside the loop of single calls it replaces, on one MI355X.
Device-resident planted pair lists (tests/fundamental_cases.py / ransac_cases.py plant them, set k with its own seed),
tol 2, N = 1024 hypotheses, PSX_RANSAC_REFIT, inlier records into a device buffer (the _dev forms):
  many   psx_ransac_<model>_many_dev( P_0 .. P_K-1 )                 one call
  loop   psx_ransac_<model>_dev( P_k ) for k = 0 .. K-1              K calls -- code this change does not touch: the baseline
run ALTERNATELY in one process (many, loop, many, loop, ...): best of 5 after 2 warm-up rounds, host wall ms per
synchronous call (for the loop: per K calls), the worst of the 5 in brackets.  Both models; K x n = 64 x 500, 16 x 1000,
8 x 4000, 1 x 1000.  Every (model, shape) is a step of its own: a child process under `timeout`, and the first step that
fails ends the run.  The results of the two forms are compared before a time is reported.
--lib PATH (in front of everything else) times another build of libpopsift_hip.so; given more than once, the builds are loaded
into ONE process and alternate round by round, one line per build: the A/B of a change to the shared kernels.  Every
build's results are compared with the first one's.
usage: python tools/ransac_many_ms.py [--lib PATH]... [out.txt]                      (default profiles/ransac_many_ms.txt)
       python tools/ransac_many_ms.py [--lib PATH]... --step MODEL K N_PAIRS          (one step: prints its line or lines)"""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 500), (16, 1000), (8, 4000), (1, 1000)]
MODELS = ("homography", "fundamental")
REPS, WARM = 5, 2
HYPOTHESES = 1024
STEP_SECONDS = 180
FMT = "%-12s %-10s %12.3f [%7.3f] %12.3f [%7.3f] %8.2fx %9d"


def bound(capi, path):
    """capi's bindings on the build at `path` (None: the tree's own); every call gives a library object of its own"""
    if path is not None:
        capi.LIB_PATH = os.path.abspath(path)
    capi._LIB = None
    return capi.lib()


def step(model, k, n, paths):
    import numpy as np

    from popsift_amd import capi
    from tests import fundamental_cases as fc
    from tests import ransac_cases as rc

    lists, lxys, rxys, off = [], [], [], 0
    for s in range(k):
        pairs, lxy, rxy = (fc.planted(n, 100 + s, fc.KINDS[s % 2]) if model == "fundamental" else rc.planted(n, 100 + s))[:3]
        p = pairs.copy()
        p["left"] += off
        off += n
        lists.append(p)
        lxys.append(lxy)
        rxys.append(rxy)
    sc, lens = np.full(k, n, np.int32), np.full(k, n, np.int32)
    opts = capi.ransac_opts(2.0, HYPOTHESES, 1, True)

    def forms(L):
        """the two forms on build L, with device buffers of its own: [many, loop, results of many, of loop, count, buffers]"""
        bufs = []
        ptrs = capi._to_device(L, 0, [np.ascontiguousarray(np.concatenate(lxys), np.float32), np.concatenate(lists)] + rxys +
                               [np.zeros((k * n, 4), np.int32)], bufs)
        plx, ppairs, prx, out = ptrs[0], ptrs[1], ptrs[2:2 + k], ptrs[2 + k]
        pa = (C.c_void_p * k)(*[p.value for p in prx])
        res_many, res_loop = (capi.RansacResult * k)(), (capi.RansacResult * k)()
        cnt = C.c_int()
        many_fn, one_fn = getattr(L, "psx_ransac_%s_many_dev" % model), getattr(L, "psx_ransac_%s_dev" % model)

        def many():
            assert many_fn(0, ppairs, sc.ctypes.data, k, plx, k * n, pa, lens.ctypes.data, C.byref(opts), res_many, out, k * n, C.byref(cnt), None, None) == 0

        def loop():
            c = C.c_int()
            for s in range(k):
                assert one_fn(0, C.c_void_p(ppairs.value + 16 * n * s), n, plx, k * n, prx[s], n, C.byref(opts), C.byref(res_loop[s]), out, n, C.byref(c),
                              None, None) == 0

        return [many, loop, res_many, res_loop, cnt, bufs]

    builds = [(L, forms(L), {"many": [], "loop": []}) for L in [bound(capi, p) for p in paths or [None]]]
    for r in range(WARM + REPS):
        for name in ("many", "loop"):
            for L, f, ts in builds:                               # with several builds: many A, many B, loop A, loop B, ...
                t0 = time.perf_counter()
                f[0 if name == "many" else 1]()
                if r >= WARM:
                    ts[name].append((time.perf_counter() - t0) * 1e3)
    for (L, f, ts), path in zip(builds, paths or [None]):
        assert bytes(f[2]) == bytes(f[3]) == bytes(builds[0][1][2]) and f[4].value == sum(r.inliers for r in f[3])
        for p in f[5]:
            L.psx_dev_free(0, p)
        m, l = ts["many"], ts["loop"]
        print(FMT % (model, "%d x %d" % (k, n), min(m), max(m), min(l), max(l), min(l) / min(m), f[4].value) + ("  " + path if path else ""))


def main(out_path, paths):
    libs = [a for p in paths for a in ("--lib", p)]
    lines = ["ransac_many_ms: psx_ransac_<model>_many_dev beside the loop of psx_ransac_<model>_dev, tol 2, %d hypotheses, refit, device in / device out;" % HYPOTHESES,
             "alternating in one process per row, best of %d after %d warm-up rounds [worst of the %d], host wall ms" % (REPS, WARM, REPS), "",
             "%-12s %-10s %22s %22s %9s %9s" % ("model", "K x n", "one call", "loop of K calls", "loop/one", "inliers")]
    status = 0
    for model in MODELS:
        for k, n in SHAPES:
            p = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__)] + libs +
                               ["--step", model, str(k), str(n)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            lines.append(p.stdout.rstrip())
            print(lines[-1], flush=True)
            status = p.returncode
            if status != 0:                                   # nothing more is started on a device after a failing step
                lines.append("step %s %d x %d ended with status %d: stopped" % (model, k, n, status))
                break
        if status != 0:
            break
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out_path, "w") as f:
        f.write(text)
    return status


if __name__ == "__main__":
    args, paths = sys.argv[1:], []
    while args and args[0] == "--lib":
        paths.append(args[1])
        args = args[2:]
    if args and args[0] == "--step":
        step(args[1], int(args[2]), int(args[3]), paths)
    else:
        sys.exit(main(args[0] if args else os.path.join(ROOT, "profiles", "ransac_many_ms.txt"), paths))
