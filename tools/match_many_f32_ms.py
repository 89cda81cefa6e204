"""dev tool (GPU box): what one FLOAT one-to-many call costs beside the loop of single calls it replaces, on one MI355X.
Device-resident float descriptors, ratio 0.8 with PSX_PAIRS_MUTUAL, records into device buffers (the _dev forms):
  many   psx_match_pairs_many_dev( L, {R_0 .. R_K-1} )           one call
  loop   psx_match_pairs_dev( L, R_k ) for k = 0 .. K-1          K calls -- code this change does not touch: the baseline
run ALTERNATELY in one process (many, loop, many, loop, ...): best of 5 after 2 warm-up rounds, host wall ms per
synchronous call (for the loop: per K calls), the worst of the 5 in brackets.  Planted content as tests/match_many_cases.py
plants it (half of every right set's rows are noisy copies of left rows), every row L2-normalised to norm 512.
Shapes: 2048 x (64 x 2048), 4096 x (16 x 4096), 3000 x (32 x 3000), 18 432 x (8 x 18 432), 18 432 x (1 x 18 432).
Further columns: the path the call took and how many of its timed calls fell back (psx_match_many_f32_last); the
candidates per (left, set) the prefilter left for the exact evaluation, mean and max, and the fullest segment of 32 --
from ONE call per shape in a fresh child process with POPSIFT_MATCH_STATS set (the library prints them; that call
synchronises per group and is not timed).
Run the tool a second time in a fresh process with POPSIFT_MATCH_MFMA=0 for path A's column (the loop then scans too).
--parent-lib PATH: also alternates psx_match_pairs_dev at 18 432 x 18 432 between this library and another build of it
(the parent commit's): the A/B of a change that touches match.hip.
usage: python tools/match_many_f32_ms.py [--parent-lib PATH] [out.txt]      (default profiles/match_many_f32_ms.txt)"""
import ctypes as C
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi

args = sys.argv[1:]
PARENT = None
STATS_CHILD = "--stats-child" in args
if STATS_CHILD:
    args.remove("--stats-child")
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    PARENT = args[i + 1]
    del args[i:i + 2]
OUT = args[0] if args else os.path.join(ROOT, "profiles", "match_many_f32_ms.txt")
SHAPES = [(2048, 64, 2048), (4096, 16, 4096), (3000, 32, 3000), (18432, 8, 18432), (18432, 1, 18432)]
REPS, WARM = 5, 2
AMPS = np.array([2, 8, 16, 24, 32, 40])


def norm512(a):
    f = a.astype(np.float32)
    n = np.sqrt((f * f).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return np.ascontiguousarray(f / n[:, None] * np.float32(512.0), np.float32)


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
        rights.append(norm512(right))
    return norm512(left), rights


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
MFMA = os.environ.get("POPSIFT_MATCH_MFMA", "1") != "0"

# the candidate statistics come from a child of their own, started before this process touches the device
stats = {}
if not STATS_CHILD and MFMA:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--stats-child"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           env=dict(os.environ, POPSIFT_MATCH_STATS="1"))
    for m in re.finditer(r"psx_match_pairs_many prefilter: (\d+) x (\d+) in (\d+) sets, candidates per \(left, set\): mean ([\d.]+), max (\d+); "
                         r"fullest segment (\d+) of (\d+)", child.stderr):
        stats[(int(m.group(1)), int(m.group(3)), int(m.group(2)) // int(m.group(3)))] = (float(m.group(4)), int(m.group(5)), int(m.group(6)))

lines = ["match_many_f32_ms: psx_match_pairs_many_dev beside the loop of psx_match_pairs_dev, ratio 0.8, mutual, device in / device out;",
         "alternating in one process, best of %d after %d warm-up rounds [worst of the %d], host wall ms; POPSIFT_MATCH_MFMA %s" %
         (REPS, WARM, REPS, "on (default)" if MFMA else "= 0 (path A; the loop scans too)"), "",
         "%-22s %22s %22s %9s %10s %5s %10s %26s" % ("left x (K x right)", "one call", "loop of K calls", "loop/one", "pairs", "path", "fell back",
                                                     "candidates mean / max / seg")]
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
    seen = {"calls": 0, "fell": 0, "path": 0}

    def many():
        assert L.psx_match_pairs_many_dev(0, pl, nl, pa, lens.ctypes.data, k, C.byref(o), out, k * nl, counts.ctypes.data, C.byref(n)) == 0
        info = capi.match_many_f32_last()
        seen["calls"] += 1; seen["fell"] += info["fell_back"]; seen["path"] = info["path"]

    if STATS_CHILD:
        many()
        for p in bufs:
            L.psx_dev_free(0, p)
        continue

    def loop():
        c = C.c_int()
        for s in range(k):
            assert L.psx_match_pairs_dev(0, pl, nl, pr[s], nr, C.byref(o), out, nl, C.byref(c)) == 0
            loop_counts[s] = c.value

    t = alternate({"many": many, "loop": loop})
    assert np.array_equal(counts, loop_counts) and n.value == counts.sum()
    st = stats.get((nl, k, nr))
    lines.append("%-22s %12.3f [%7.3f] %12.3f [%7.3f] %8.2fx %10d %5d %6d/%-3d %26s" %
                 ("%d x (%d x %d)" % (nl, k, nr), t["many"][0], t["many"][1], t["loop"][0], t["loop"][1], t["loop"][0] / t["many"][0], n.value,
                  seen["path"], seen["fell"], seen["calls"], "%.1f / %d / %d of 32" % st if st else "-"))
    if PARENT and (nl, k, nr) == (18432, 1, 18432):
        P = C.CDLL(PARENT)
        for lib in (P, L):
            lib.psx_match_pairs_dev.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(capi.MatchOpts), C.c_void_p, C.c_int,
                                                C.POINTER(C.c_int)]
        c = C.c_int()

        def single(lib):
            assert lib.psx_match_pairs_dev(0, pl, nl, pr[0], nr, C.byref(o), out, nl, C.byref(c)) == 0

        ab = alternate({"parent": lambda: single(P), "this": lambda: single(L)})
        lines += ["", "psx_match_pairs_dev at 18432 x 18432, the parent commit's library and this one alternating in one process:",
                  "  parent %.3f [%.3f]   this %.3f [%.3f]" % (ab["parent"][0], ab["parent"][1], ab["this"][0], ab["this"][1])]
        P.psx_match_release()
    for p in bufs:
        L.psx_dev_free(0, p)
if STATS_CHILD:
    sys.exit(0)
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)
