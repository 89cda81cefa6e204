"""dev tool (GPU box): what one one-to-many call costs beside the loop of single calls it replaces, on one MI355X.
Device-resident byte descriptors, ratio 0.8 with PSX_PAIRS_MUTUAL, records into device buffers (the _dev forms):
  many   psx_match_pairs_many_u8_dev( L, {R_0 .. R_K-1} )           one call
  loop   psx_match_pairs_u8_dev( L, R_k ) for k = 0 .. K-1          K calls -- code this change does not touch: the baseline
run ALTERNATELY in one process (many, loop, many, loop, ...): best of 5 after 2 warm-up rounds, host wall ms per
synchronous call (for the loop: per K calls), the worst of the 5 in brackets.  Planted content as tests/match_many_cases.py
plants it: half of every right set's rows are noisy copies of left rows.  Shapes: 2048 x (64 x 2048), 4096 x (16 x 4096),
18 432 x (8 x 18 432), 18 432 x (1 x 18 432).
--parent-lib PATH: also alternates psx_match_pairs_u8_dev at 18 432 x 18 432 between this library and another build of it
(the parent commit's): the A/B of a change that touches match.hip.
usage: python tools/match_many_ms.py [--parent-lib PATH] [out.txt]      (default profiles/match_many_ms.txt)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi

args = sys.argv[1:]
PARENT = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    PARENT = args[i + 1]
    del args[i:i + 2]
OUT = args[0] if args else os.path.join(ROOT, "profiles", "match_many_ms.txt")
SHAPES = [(2048, 64, 2048), (4096, 16, 4096), (18432, 8, 18432), (18432, 1, 18432)]
REPS, WARM = 5, 2
AMPS = np.array([2, 8, 16, 24, 32, 40])


def sets(seed, nl, k, nr):
    left = np.random.default_rng(seed).integers(0, 64, (nl, 128), dtype=np.uint8)
    rights = []
    for s in range(k):
        rng = np.random.default_rng([seed, s + 1])
        right = rng.integers(0, 64, (nr, 128), dtype=np.uint8)
        m = min(nl, nr) // 2
        src, dst = rng.permutation(nl)[:m], rng.permutation(nr)[:m]
        amp = AMPS[np.arange(m) % 6][:, None]
        noise = (rng.random((m, 128)) * (2 * amp + 1)).astype(np.int64) - amp
        right[dst] = np.clip(left[src].astype(np.int64) + noise, 0, 255).astype(np.uint8)
        rights.append(right)
    return left, rights


def alternate(calls):
    """calls: name -> function; every round runs each once, in order; (best, worst) of the REPS rounds after WARM"""
    ts = {n: [] for n in calls}
    for r in range(WARM + REPS):
        for n, f in calls.items():
            t0 = time.perf_counter()
            f()
            if r >= WARM:
                ts[n].append((time.perf_counter() - t0) * 1e3)
    return {n: (min(v), max(v)) for n, v in ts.items()}


L = capi.lib()
o = capi.match_opts(0.8, True)
lines = ["match_many_ms: psx_match_pairs_many_u8_dev beside the loop of psx_match_pairs_u8_dev, ratio 0.8, mutual, device in / device out;",
         "alternating in one process, best of %d after %d warm-up rounds [worst of the %d], host wall ms" % (REPS, WARM, REPS), "",
         "%-22s %22s %22s %9s %10s" % ("left x (K x right)", "one call", "loop of K calls", "loop/one", "pairs")]
for nl, k, nr in SHAPES:
    left, rights = sets(nl + k, nl, k, nr)
    bufs = []
    ptrs = capi._to_device(L, 0, [left] + rights, bufs)
    pl, pr = ptrs[0], ptrs[1:]
    out = capi._to_device(L, 0, [np.zeros((k * nl, 4), np.int32)], bufs)[0]
    pa = (C.c_void_p * k)(*[p.value for p in pr])
    lens = np.full(k, nr, np.int32)
    counts = np.zeros(k, np.int32)
    n = C.c_int()
    loop_counts = np.zeros(k, np.int32)

    def many():
        assert L.psx_match_pairs_many_u8_dev(0, pl, nl, pa, lens.ctypes.data, k, C.byref(o), out, k * nl, counts.ctypes.data, C.byref(n)) == 0

    def loop():
        c = C.c_int()
        for s in range(k):
            assert L.psx_match_pairs_u8_dev(0, pl, nl, pr[s], nr, C.byref(o), out, nl, C.byref(c)) == 0
            loop_counts[s] = c.value

    t = alternate({"many": many, "loop": loop})
    assert np.array_equal(counts, loop_counts) and n.value == counts.sum()
    lines.append("%-22s %12.3f [%7.3f] %12.3f [%7.3f] %8.2fx %10d" % ("%d x (%d x %d)" % (nl, k, nr), t["many"][0], t["many"][1],
                                                                     t["loop"][0], t["loop"][1], t["loop"][0] / t["many"][0], n.value))
    if PARENT and (nl, k, nr) == (18432, 1, 18432):
        P = C.CDLL(PARENT)
        for lib in (P, L):
            lib.psx_match_pairs_u8_dev.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(capi.MatchOpts), C.c_void_p, C.c_int,
                                                   C.POINTER(C.c_int)]
        c = C.c_int()

        def single(lib):
            assert lib.psx_match_pairs_u8_dev(0, pl, nl, pr[0], nr, C.byref(o), out, nl, C.byref(c)) == 0

        ab = alternate({"parent": lambda: single(P), "this": lambda: single(L)})
        lines += ["", "psx_match_pairs_u8_dev at 18432 x 18432, the parent commit's library and this one alternating in one process:",
                  "  parent %.3f [%.3f]   this %.3f [%.3f]" % (ab["parent"][0], ab["parent"][1], ab["this"][0], ab["this"][1])]
        P.psx_match_release()
    for p in bufs:
        L.psx_dev_free(0, p)
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)
