"""Byte descriptors against float descriptors on one box (GPU).

  python tools/byte_desc_ab.py [--frames N] [--pairs P] [--out FILE]

1. Extraction through the C-ABI at the headline frame size (1920x1080, VLFeat, the bench's 4 octaves), one context per
   format, frames run back to back (upload, extract, results on the host): float mode with psx_download against byte
   mode with psx_download_u8, and the same with the zero-copy export attached (psx_attach_export /
   psx_attach_export_u8).  The legs alternate in pairs; Mpix/s per leg and pair.
2. psx_match_u8 against psx_match at 18432 x 18432 on the same byte-valued inputs (device resident), best of 10 calls.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from popsift_amd import capi  # noqa: E402
from popsift_amd.synth import synth  # noqa: E402


def run_leg(ctx, frames, fmt, export, bufs):
    t0 = time.perf_counter()
    for img in frames:
        ctx.upload(img)
        ctx.extract()
        if export:
            ctx.counts()
        elif fmt == capi.DESCFMT_U8:
            ctx.download_u8()
        else:
            ctx.download()
    dt = time.perf_counter() - t0
    return len(frames) * img.size / dt / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    frames = [synth(1920, 1080, 1000 + i) for i in range(8)]
    frames = (frames * ((a.frames + 7) // 8))[: a.frames]
    cfg = capi.default_config(octaves=4, sift_mode=2)
    res = {"frames": a.frames, "pairs": []}
    cap = 60000
    ctxs = {}
    for fmt in (capi.DESCFMT_F32, capi.DESCFMT_U8):
        for export in (False, True):
            ctx = capi.Context(cfg)
            ctx.set_descriptor_format(fmt)
            fb = np.zeros(cap * capi.FEATURE_DTYPE.itemsize, np.uint8)
            db = np.zeros((cap, 128), np.uint8 if fmt == capi.DESCFMT_U8 else np.float32)
            if export:
                (ctx.attach_export_u8 if fmt == capi.DESCFMT_U8 else ctx.attach_export)(fb, db)
            run_leg(ctx, frames[:4], fmt, export, None)          # warm-up
            ctxs[(fmt, export)] = (ctx, fb, db)
    for p in range(a.pairs):
        row = {}
        for export in (False, True):
            order = (capi.DESCFMT_F32, capi.DESCFMT_U8) if p % 2 == 0 else (capi.DESCFMT_U8, capi.DESCFMT_F32)
            for fmt in order:
                ctx = ctxs[(fmt, export)][0]
                row["%s_%s" % ("u8" if fmt else "f32", "export" if export else "download")] = round(run_leg(ctx, frames, fmt, export, None), 1)
        res["pairs"].append(row)
        print(json.dumps(row), flush=True)
    for v in ctxs.values():
        v[0].close()

    # matcher
    rng = np.random.default_rng(7)
    left = rng.integers(0, 256, size=(18432, 128), dtype=np.uint8)
    right = rng.integers(0, 256, size=(18432, 128), dtype=np.uint8)
    right[:4096] = np.clip(left[:4096].astype(np.int32) + rng.integers(-3, 4, size=(4096, 128)), 0, 255).astype(np.uint8)
    L = capi.lib()
    L.psx_match_u8.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.psx_match.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    bufs = []
    try:
        pl, pr, plf, prf = capi._to_device(L, 0, [left, right, left.astype(np.float32), right.astype(np.float32)], bufs)
        mm = np.zeros((18432, 3), np.int32); dd = np.zeros((18432, 2), np.int32)
        mf = np.zeros((18432, 3), np.int32); df = np.zeros((18432, 2), np.float32)
        tu, tf = [], []
        for _ in range(10):
            t0 = time.perf_counter(); L.psx_match_u8(0, pl, 18432, pr, 18432, mm.ctypes.data, dd.ctypes.data); tu.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); L.psx_match(0, plf, 18432, prf, 18432, mf.ctypes.data, df.ctypes.data); tf.append(time.perf_counter() - t0)
        assert np.array_equal(mm, mf), "matchers disagree"
        res["match_18432_ms"] = {"psx_match_u8": round(1e3 * min(tu), 3), "psx_match": round(1e3 * min(tf), 3)}
    finally:
        for q in bufs:
            L.psx_dev_free(0, q)
    print(json.dumps(res["match_18432_ms"]))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
