"""dev tool (GPU box): what geometric verification costs, psx_ransac_homography_dev and psx_ransac_fundamental_dev on one
MI355X.  20 000 pairs x 4096 hypotheses, pairs and inliers in device memory; per setting BATCHES batches of 30 synchronous
calls after 3 warm-up calls, host wall time of the call; reported: the median of the batch medians and their spread
(max - min), which is what two builds of the same code differ by.  Beside it the host reference (psx_ransac_*_ref, one
thread, one call).  60 % of the pairs are planted: under a homography for the homography estimator, on a scene with depth
(two cameras) for the fundamental matrix; the others are uniform outliers.
--lib PATH times another build of libpopsift_hip.so (an older one without the fundamental entry points is timed on the
homography alone); given more than once, the builds are loaded into ONE process and their batches alternate, which is the
A/B of a change to the shared kernels: the results of the later builds are compared with the first one's.
usage: python tools/ransac_ms.py [--lib PATH]... [--pairs 20000] [--hypotheses 4096] [--batches 5] [--no-ref] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append")
ap.add_argument("--pairs", type=int, default=20000)
ap.add_argument("--hypotheses", type=int, default=4096)
ap.add_argument("--batches", type=int, default=5)
ap.add_argument("--no-ref", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_ms.txt"))
args = ap.parse_args()
n, N, CALLS, WARM = args.pairs, args.hypotheses, 30, 3


class Opts(C.Structure):
    _fields_ = [("tol", C.c_float), ("hypotheses", C.c_int), ("seed", C.c_uint), ("flags", C.c_int)]


class Result(C.Structure):
    _fields_ = [("m", C.c_float * 9), ("best", C.c_int), ("sample_inliers", C.c_int), ("inliers", C.c_int), ("refit_kept", C.c_int)]


vp = C.c_void_p
DEV_ARGS = [C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(Opts), C.POINTER(Result), vp, C.c_int, C.POINTER(C.c_int), vp, vp]
REF_ARGS = DEV_ARGS[1:]
LIBS = []
for path in args.lib or [os.path.join(ROOT, "popsift_amd", "lib", "libpopsift_hip.so")]:
    L = C.CDLL(path)
    L.psx_dev_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(vp)]
    L.psx_dev_free.argtypes = [C.c_int, vp]
    L.psx_dev_write.argtypes = [C.c_int, vp, vp, C.c_size_t]
    LIBS.append((os.path.relpath(path, ROOT), L))


def upload(L, a):
    a = np.ascontiguousarray(a)
    p = vp()
    assert L.psx_dev_alloc(0, a.nbytes, C.byref(p)) == 0 and L.psx_dev_write(0, p, a.ctypes.data_as(vp), a.nbytes) == 0
    return p


def inputs(model):
    rng = np.random.default_rng(20000)
    left = rng.uniform([0, 0], [640, 480], (n, 2))
    h = np.concatenate([left, np.ones((n, 1))], 1)
    if model == "homography":
        q = h @ np.array([[1.25, 0.03, 4.0], [-0.02, 1.2, -3.0], [1e-4, -5e-5, 1.0]]).T
    else:
        K = np.array([[500., 0, 320], [0, 500., 240], [0, 0, 1]])
        a = 0.15
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        X = np.linalg.inv(K) @ h.T * rng.uniform(3, 9, n)
        q = (K @ (R @ X + np.array([-1.0, 0.1, 0.2])[:, None])).T
    right = q[:, :2] / q[:, 2:3]
    ang, rad = rng.uniform(0, 2 * np.pi, n), np.array([0.0, 0.5, 1.5])[np.arange(n) % 3]
    right += np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    out = np.arange(n) % 5 >= 3
    right[out] = rng.uniform(right.min(0), right.max(0), (n, 2))[out]
    pairs = np.zeros(n, np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<f4"), ("d2", "<f4")]))
    pairs["left"] = pairs["right"] = np.arange(n)
    return pairs, np.ascontiguousarray(left, np.float32), np.ascontiguousarray(right, np.float32)     # row major: the host reference reads them in place


def batches(calls):
    """per call: (median of its batch medians, their spread); the batches of the calls alternate"""
    meds = [[] for _ in calls]
    for _ in range(args.batches):
        for call, m in zip(calls, meds):
            ts = []
            for i in range(WARM + CALLS):
                t0 = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t0) * 1e3)
            m.append(float(np.median(ts[WARM:])))
    return [(float(np.median(m)), max(m) - min(m)) for m in meds]


lines = ["ransac_ms: %s" % ", ".join(name for name, _ in LIBS),
         "%d pairs x %d hypotheses, tol 2, device-resident pairs and inliers; %d batches of %d synchronous calls after %d warm-up "
         "calls%s: median of the batch medians [spread of the batch medians], host wall ms"
         % (n, N, args.batches, CALLS, WARM, ", the libraries' batches alternating in one process" if len(LIBS) > 1 else "")]
differs = False
for model in ("homography", "fundamental"):
    libs = [(name, L) for name, L in LIBS if hasattr(L, "psx_ransac_%s_dev" % model)]
    lines += ["%-12s not in %s" % (model, name) for name, L in LIBS if (name, L) not in libs]
    pairs, lxy, rxy = inputs(model)
    bufs = [[upload(L, a) for a in (pairs, lxy, rxy, np.zeros(n * 16, np.uint8))] for _, L in libs]
    for _, L in libs:
        getattr(L, "psx_ransac_%s_dev" % model).argtypes, getattr(L, "psx_ransac_%s_ref" % model).argtypes = DEV_ARGS, REF_ARGS
    for refit in (0, 1):
        o = Opts(2.0, N, 0, refit)
        outs = [(Result(), C.c_int()) for _ in libs]

        def caller(L, b, res, cnt):
            dev = getattr(L, "psx_ransac_%s_dev" % model)

            def call():
                assert dev(0, b[0], n, b[1], n, b[2], n, C.byref(o), C.byref(res), b[3], n, C.byref(cnt), None, None) == 0
            return call

        timed = batches([caller(L, b, res, cnt) for (_, L), b, (res, cnt) in zip(libs, bufs, outs)])
        for (name, L), (med, spread), (res, cnt) in zip(libs, timed, outs):
            text = "%-12s refit %d: device %.4f [%.4f] ms, %d inliers (sample %d, refit kept %d)" % (model, refit, med, spread, cnt.value,
                                                                                                      res.sample_inliers, res.refit_kept)
            if len(LIBS) > 1:
                text += "  " + name
            if bytes(res) != bytes(outs[0][0]) or cnt.value != outs[0][1].value:
                differs = True
                text += "\n  THE RESULT DIFFERS FROM THAT OF %s" % libs[0][0]
            if not args.no_ref:
                out = np.zeros(n * 16, np.uint8)
                r2, c2 = Result(), C.c_int()
                t0 = time.perf_counter()
                assert getattr(L, "psx_ransac_%s_ref" % model)(pairs.ctypes.data_as(vp), n, lxy.ctypes.data_as(vp), n, rxy.ctypes.data_as(vp), n, C.byref(o),
                                                               C.byref(r2), out.ctypes.data_as(vp), n, C.byref(c2), None, None) == 0
                host = (time.perf_counter() - t0) * 1e3
                text += "; host reference, one thread: %.0f ms (%.0f x)" % (host, host / med)
                if bytes(r2) != bytes(res) or c2.value != cnt.value:
                    differs = True
                    text += "\n  THE DEVICE RESULT DIFFERS FROM THE HOST REFERENCE: device %s best %d sample %d inliers %d kept %d count %d; host %s best %d sample %d inliers %d kept %d count %d" % (
                        list(res.m), res.best, res.sample_inliers, res.inliers, res.refit_kept, cnt.value,
                        list(r2.m), r2.best, r2.sample_inliers, r2.inliers, r2.refit_kept, c2.value)
            lines.append(text)
    for (_, L), b in zip(libs, bufs):
        for p in b:
            L.psx_dev_free(0, p)
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
sys.exit(1 if differs else 0)
