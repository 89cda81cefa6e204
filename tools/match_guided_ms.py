"""dev tool (GPU box): what guided matching costs beside the unconstrained pair search, 18 432 x 18 432 unit-norm float
descriptors with points uniform in 1920 x 1080, on one MI355X.  Best of 5 after 2 warm-up calls, device-resident
descriptors and positions, host wall time of the whole synchronous call, mutual pairs at ratio 0.8:
  psx_match_pairs                     the unconstrained search (the code of the parent commit, unchanged, in the same process):
                                      what a caller runs today before filtering the pairs on the host -- the yardstick
  psx_match_pairs_guided, window      identity H, tol 8: a search window of radius 8 px
  psx_match_pairs_guided, epipolar    F = [t]x, tol 2: a band of +-2 px around the epipolar line
and the admissible fraction of each guide (psx_guide_allows over all pairs).  Half of the right descriptors are noisy
copies of left ones and sit within 1 px of their partner's position, so the guided searches have pairs to find.
usage: python tools/match_guided_ms.py [n] [out.txt]      (default 18432, profiles/match_guided_ms.txt)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from popsift_amd import capi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 18432
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "match_guided_ms.txt")
REPS, WARM = 5, 2
W, H = 1920.0, 1080.0
rng = np.random.default_rng(18432)


def unit(n):
    v = rng.random((n, 128), dtype=np.float32) ** 4
    return np.sqrt(v / v.sum(1, keepdims=True)).astype(np.float32)


def best_ms(call):
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[WARM:]
    return min(ts), max(ts)


def admissible_fraction(guide, lxy, rxy):
    n = 0
    for i in range(0, len(lxy), 1024):
        n += int(capi.guide_allows(guide, lxy[i:i + 1024], rxy).sum())
    return n / (len(lxy) * len(rxy))


left, right = unit(N), unit(N)
lxy = (rng.random((N, 2)) * [W, H]).astype(np.float32)
rxy = (rng.random((N, 2)) * [W, H]).astype(np.float32)
src, dst = rng.permutation(N)[:N // 2], rng.permutation(N)[:N // 2]
scale = (np.float32(0.01) * (1 + np.arange(N // 2) % 6)).astype(np.float32)[:, None]
right[dst] = left[src] + (rng.random((N // 2, 128), dtype=np.float32) - np.float32(0.5)) * scale
rxy[dst] = lxy[src] + (rng.random((N // 2, 2)) * 2 - 1).astype(np.float32)

t = (1.0, 0.02, 0.0001)
guides = [("window (identity H, tol 8)", capi.Guide.homography([1, 0, 0, 0, 1, 0, 0, 0, 1], 8.0)),
          ("epipolar band (F = [t]x, tol 2)", capi.Guide.epipolar([0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0], 2.0))]

L = capi.lib()
bufs = []
pl, plx, pr, prx = capi._to_device(L, 0, [left, lxy, right, rxy], bufs)
pairs = np.zeros((N,), capi.PAIR_DTYPE)
cnt = C.c_int()
opts = capi.match_opts(0.8, True)


def run_plain():
    assert L.psx_match_pairs(0, pl, N, pr, N, C.byref(opts), pairs.ctypes.data, N, C.byref(cnt)) == 0


def run_guided(g):
    assert L.psx_match_pairs_guided(0, pl, plx, N, pr, prx, N, C.byref(g), C.byref(opts), pairs.ctypes.data, N, C.byref(cnt)) == 0


lines = ["match_guided_ms: %d x %d unit-norm float descriptors, points uniform in %d x %d, mutual pairs at ratio 0.8;" % (N, N, W, H),
         "best of %d after %d warm-up calls (max of the %d in brackets), host wall ms per synchronous call" % (REPS, WARM, REPS), ""]
ref = best_ms(run_plain)
lines.append("  %-44s %.3f [%.3f]   %d pairs   <- the yardstick (unconstrained, unchanged code)" % ("psx_match_pairs", ref[0], ref[1], cnt.value))
for name, g in guides:
    ms = best_ms(lambda: run_guided(g))
    n = cnt.value
    frac = admissible_fraction(g, lxy, rxy)
    lines.append("  %-44s %.3f [%.3f]   %d pairs, admissible fraction %.3e (%.1f rights per left), %.2f x the yardstick"
                 % ("psx_match_pairs_guided " + name, ms[0], ms[1], n, frac, frac * N, ms[0] / ref[0]))
again = best_ms(run_plain)
lines.append("  %-44s %.3f [%.3f]   (the yardstick again, after the guided calls)" % ("psx_match_pairs", again[0], again[1]))
for p in bufs:
    L.psx_dev_free(0, p)
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)
