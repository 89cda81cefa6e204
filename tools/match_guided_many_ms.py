"""dev tool (GPU box): what one guided one-to-many call costs beside the loop of single guided calls it replaces, on one
MI355X.  Device-resident byte descriptors with positions, ratio 0.8 with PSX_PAIRS_MUTUAL, records into device buffers
(the _dev forms):
  many   psx_match_pairs_guided_many_u8_dev( L, {R_0 .. R_K-1}, {guide_0 .. guide_K-1} )      one call
  loop   psx_match_pairs_guided_u8_dev( L, R_k, guide_k ) for k = 0 .. K-1                    K calls -- code this change
                                                                                              does not touch: the baseline
run ALTERNATELY in one process (many, loop, many, loop, ...): median of 5 after 2 warm-up rounds, host wall ms per
synchronous call (for the loop: per K calls), the worst of the 5 in brackets.  K = 1, 8, 64 sets of 2048 and of 4096 rows
against a left set of the same length.  Points uniform in 1920 x 1080; half of every right set's rows are noisy copies of
left rows (as tests/match_many_cases.py plants them) within 1 px of their left point.  Two guides:
  window   identity H, the radius chosen so that a left point has about 2.5 admissible right points (the first row of
           profiles/match_guided_ms.txt: 2.3 per left)
  band     the epipolar band of a horizontal motion, F = [t]x with t = (1, 0, 0), tol 2: |yr - yl| <= 2 px
usage: python tools/match_guided_many_ms.py [out.txt]      (default profiles/match_guided_many_ms.txt)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi

args = sys.argv[1:]
OUT = args[0] if args else os.path.join(ROOT, "profiles", "match_guided_many_ms.txt")
W, H = 1920.0, 1080.0
SHAPES = [(n, k) for n in (2048, 4096) for k in (1, 8, 64)]
REPS, WARM = 5, 2
AMPS = np.array([2, 8, 16, 24, 32, 40])
IDENT = (1, 0, 0, 0, 1, 0, 0, 0, 1)
F_ROWS = (0, 0, 0, 0, 0, -1, 0, 1, 0)


def sets(seed, nl, k, nr):
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 64, (nl, 128), dtype=np.uint8)
    lxy = rng.uniform((0, 0), (W, H), (nl, 2))
    rights, rxys = [], []
    for s in range(k):
        rng = np.random.default_rng([seed, s + 1])
        right = rng.integers(0, 64, (nr, 128), dtype=np.uint8)
        rxy = rng.uniform((0, 0), (W, H), (nr, 2))
        m = min(nl, nr) // 2
        src, dst = rng.permutation(nl)[:m], rng.permutation(nr)[:m]
        amp = AMPS[np.arange(m) % 6][:, None]
        noise = (rng.random((m, 128)) * (2 * amp + 1)).astype(np.int64) - amp
        right[dst] = np.clip(left[src].astype(np.int64) + noise, 0, 255).astype(np.uint8)
        rxy[dst] = lxy[src] + rng.uniform(-0.7, 0.7, (m, 2))
        rights.append(right)
        rxys.append(rxy.astype(np.float32))
    return left, lxy.astype(np.float32), rights, rxys


def alternate(calls):
    """calls: name -> function; every round runs each once, in order; (median, worst) of the REPS rounds after WARM"""
    ts = {n: [] for n in calls}
    for r in range(WARM + REPS):
        for n, f in calls.items():
            t0 = time.perf_counter()
            f()
            if r >= WARM:
                ts[n].append((time.perf_counter() - t0) * 1e3)
    return {n: (float(np.median(v)), max(v)) for n, v in ts.items()}


L = capi.lib()
o = capi.match_opts(0.8, True)
lines = ["match_guided_many_ms: psx_match_pairs_guided_many_u8_dev beside the loop of psx_match_pairs_guided_u8_dev, ratio 0.8, mutual,",
         "device in / device out; alternating in one process, median of %d after %d warm-up rounds [worst of the %d], host wall ms" % (REPS, WARM, REPS),
         "", "%-8s %-22s %10s %22s %22s %9s %10s" % ("guide", "left x (K x right)", "adm./left", "one call", "loop of K calls", "loop/one", "pairs")]
for nl, k in SHAPES:
    nr = nl
    left, lxy, rights, rxys = sets(nl + k, nl, k, nr)
    bufs = []
    ptrs = capi._to_device(L, 0, [left, lxy] + rights + rxys, bufs)
    pl, plx, pr, prx = ptrs[0], ptrs[1], ptrs[2:2 + k], ptrs[2 + k:]
    out = capi._to_device(L, 0, [np.zeros((k * nl, 4), np.int32)], bufs)[0]
    pa = (C.c_void_p * k)(*[p.value for p in pr])
    xa = (C.c_void_p * k)(*[p.value for p in prx])
    lens = np.full(k, nr, np.int32)
    radius = float(np.sqrt(2.5 * W * H / (np.pi * nr)))
    for name, guide in (("window", capi.Guide.homography(IDENT, radius)), ("band", capi.Guide.epipolar(F_ROWS, 2.0))):
        ga = (capi.Guide * k)(*[guide] * k)
        counts = np.zeros(k, np.int32)
        n = C.c_int()
        loop_counts = np.zeros(k, np.int32)

        def many():
            assert L.psx_match_pairs_guided_many_u8_dev(0, pl, plx, nl, pa, xa, lens.ctypes.data, k, ga, C.byref(o), out, k * nl,
                                                        counts.ctypes.data, C.byref(n)) == 0

        def loop():
            c = C.c_int()
            for s in range(k):
                assert L.psx_match_pairs_guided_u8_dev(0, pl, plx, nl, pr[s], prx[s], nr, C.byref(guide), C.byref(o), out, nl, C.byref(c)) == 0
                loop_counts[s] = c.value

        t = alternate({"many": many, "loop": loop})
        assert np.array_equal(counts, loop_counts) and n.value == counts.sum()
        adm = capi.guide_allows(guide, lxy[:256], rxys[0]).sum(1).mean()
        lines.append("%-8s %-22s %10.1f %12.3f [%7.3f] %12.3f [%7.3f] %8.2fx %10d" %
                     (name, "%d x (%d x %d)" % (nl, k, nr), adm, t["many"][0], t["many"][1], t["loop"][0], t["loop"][1],
                      t["loop"][0] / t["many"][0], n.value))
    for p in bufs:
        L.psx_dev_free(0, p)
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)
