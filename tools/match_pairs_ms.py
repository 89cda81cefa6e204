"""dev tool (GPU box): what the pair search costs beside the directed matcher, 18 432 x 18 432 on one MI355X, bytes and floats.
Best of 5 after 2 warm-up calls, device-resident descriptors, host wall time of the whole synchronous call:
  psx_match(_u8) L -> R, R -> L, their sum (the yardstick: the parent commit's code, in the same process),
  psx_match_pairs(_u8) directed ({0.8, 0}) and mutual ({0.8, PSX_PAIRS_MUTUAL}),
and the bytes each copies back.  A host that wants mutual pairs today pays the sum plus its own join.
usage: python tools/match_pairs_ms.py [n] [out.txt]      (default 18432, profiles/match_pairs_ms.txt)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from popsift_amd import capi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 18432
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "match_pairs_ms.txt")
REPS, WARM = 5, 2
rng = np.random.default_rng(18432)


def byte_sets():
    left = rng.integers(0, 64, (N, 128), dtype=np.uint8)
    right = rng.integers(0, 64, (N, 128), dtype=np.uint8)
    src, dst = rng.permutation(N)[:N // 2], rng.permutation(N)[:N // 2]
    amp = np.array([2, 8, 16, 24, 32, 40])[np.arange(N // 2) % 6][:, None]
    noise = (rng.random((N // 2, 128)) * (2 * amp + 1)).astype(np.int64) - amp
    right[dst] = np.clip(left[src].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return left, right


def float_sets():
    def unit(n):
        v = rng.random((n, 128), dtype=np.float32) ** 4
        return np.sqrt(v / v.sum(1, keepdims=True)).astype(np.float32)
    left, right = unit(N), unit(N)
    src, dst = rng.permutation(N)[:N // 2], rng.permutation(N)[:N // 2]
    scale = (np.float32(0.01) * (1 + np.arange(N // 2) % 6)).astype(np.float32)[:, None]
    right[dst] = left[src] + (rng.random((N // 2, 128), dtype=np.float32) - np.float32(0.5)) * scale
    return left, right


def best_ms(call):
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[WARM:]
    return min(ts), max(ts)


L = capi.lib()
lines = ["match_pairs_ms: %d x %d descriptors, best of %d after %d warm-up calls (max of the %d in brackets), host wall ms per synchronous call" % (N, N, REPS, WARM, REPS)]
for kind, (left, right) in (("bytes", byte_sets()), ("floats", float_sets())):
    u8 = kind == "bytes"
    bufs = []
    pl, pr = capi._to_device(L, 0, [left, right], bufs)
    mm = np.zeros((N, 3), np.int32)
    dd = np.zeros((N, 2), np.int32 if u8 else np.float32)
    pairs = np.zeros((N,), capi.PAIR_U8_DTYPE if u8 else capi.PAIR_DTYPE)
    cnt = C.c_int()
    directed = L.psx_match_u8 if u8 else L.psx_match
    pairs_fn = L.psx_match_pairs_u8 if u8 else L.psx_match_pairs
    directed.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

    def run_directed(a, b):
        assert directed(0, a, N, b, N, mm.ctypes.data, dd.ctypes.data) == 0

    def run_pairs(o):
        assert pairs_fn(0, pl, N, pr, N, C.byref(o), pairs.ctypes.data, N, C.byref(cnt)) == 0

    lr = best_ms(lambda: run_directed(pl, pr))
    rl = best_ms(lambda: run_directed(pr, pl))
    o_dir, o_mut = capi.match_opts(0.8, False), capi.match_opts(0.8, True)
    pd = best_ms(lambda: run_pairs(o_dir))
    n_dir = cnt.value
    pm = best_ms(lambda: run_pairs(o_mut))
    n_mut = cnt.value
    name = "psx_match_u8" if u8 else "psx_match"
    lines += ["", "%s:" % kind,
              "  %-34s %.3f [%.3f]   copies back %d B" % (name + " L->R", lr[0], lr[1], 20 * N),
              "  %-34s %.3f [%.3f]   copies back %d B" % (name + " R->L", rl[0], rl[1], 20 * N),
              "  %-34s %.3f           copies back %d B   <- the yardstick; spread of the directed runs %.3f" %
              ("sum of the two", lr[0] + rl[0], 40 * N, max(lr[1] - lr[0], rl[1] - rl[0])),
              "  %-34s %.3f [%.3f]   %d pairs, copies back %d B" % (name.replace("match", "match_pairs") + " directed", pd[0], pd[1], n_dir, 4 + 16 * n_dir),
              "  %-34s %.3f [%.3f]   %d pairs, copies back %d B" % (name.replace("match", "match_pairs") + " mutual", pm[0], pm[1], n_mut, 4 + 16 * n_mut)]
    for p in bufs:
        L.psx_dev_free(0, p)
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)
