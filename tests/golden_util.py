"""Load the committed reference fixtures (tests/golden/ref_*.npz, made by tests/golden/make_golden.py
from the reference's own code running on the CPU)."""
import glob
import hashlib
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cases():
    return sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "ref_*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, "ref_%s.npz" % name), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config"]))
    d["plane_sha1"] = json.loads(str(d["plane_sha1"]))
    d["dims"] = [tuple(int(v) for v in row) for row in d["dims"]]
    d["num_levels"] = int(d["num_levels"])
    return d


def sha1(plane):
    return hashlib.sha1(np.ascontiguousarray(plane, dtype=np.float32).tobytes()).hexdigest()


def big_cases():
    return sorted(os.path.basename(p)[7:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "bigref_*.npz")))


def load_big(name):
    """Full-size fixtures (make_golden.py BIG_CASES): the image is regenerated from its seed (its SHA-1 is checked),
    every plane is a SHA-1, all Feature records are kept, and every desc_stride-th descriptor."""
    from popsift_amd.synth import synth
    z = np.load(os.path.join(GOLDEN_DIR, "bigref_%s.npz" % name), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config"]))
    d["plane_sha1"] = json.loads(str(d["plane_sha1"]))
    d["dims"] = [tuple(int(v) for v in row) for row in d["dims"]]
    d["num_levels"] = int(d["num_levels"])
    w, h = (int(v) for v in d["size"])
    d["image"] = synth(w, h, int(d["seed"]))
    assert hashlib.sha1(d["image"].tobytes()).hexdigest() == str(d["image_sha1"]), "synth() no longer reproduces the fixture's image"
    d["desc_stride"] = int(d["desc_stride"])
    d["desc_count"] = int(d["desc_count"])
    return d


# ---- tests/test_ref_shim_cpu.py: the reference's answers to exactly the calls that module makes -------------------------
# one file per test function: refshim/<test name>.npz
REFSHIM_DIR = os.path.join(GOLDEN_DIR, "refshim")


def _key(kind, *parts):
    """Name of one call of the reference: its kind and a digest of its arguments (images, descriptor sets, Config fields)."""
    h = hashlib.sha1(kind.encode())
    for p in parts:
        if isinstance(p, np.ndarray):
            p = np.ascontiguousarray(p)
            h.update(repr((p.dtype.str, p.shape)).encode())
            h.update(p.tobytes())
        elif hasattr(p, "_fields_"):
            h.update(repr([(f[0], getattr(p, f[0])) for f in p._fields_]).encode())
        else:
            h.update(repr(p).encode())
    return kind + "_" + h.hexdigest()[:20]


def plane_digest(plane):
    """What a reference plane is compared by: a replayed one already is its digest, a computed one is hashed."""
    return plane if isinstance(plane, str) else "%s %s" % (tuple(np.shape(plane)), sha1(plane))


class ReferenceRecorder:
    """Passes the calls of tests/test_ref_shim_cpu.py to the live reference (oracle/pyref.py) and keeps every answer the
    tests read (tests/golden/make_refshim.py)."""

    def __init__(self, live):
        self.live, self.data = live, {}

    def gauss_tables(self, cfg):
        t = self.live.gauss_tables(cfg)
        k = _key("tables", cfg)
        self.data.update({"%s.%s" % (k, n): np.array(v) for n, v in t.items()})
        return t

    def match(self, left, right):
        mm, dd = self.live.match(left, right)
        k = _key("match", left, right)
        self.data.update({k + ".mm": mm.copy(), k + ".dd": dd.copy()})
        return mm, dd

    def run(self, cfg, img, api=False):
        r = self.live.run(cfg, img, api=api)
        k = _key("run", cfg, img, api)
        no, nl = r.num_octaves, r.num_levels
        meta = {"num_octaves": no, "num_levels": nl, "dims": r.dims, "ext_total": r.ext_total, "ori_total": r.ori_total,
                "gauss": [[plane_digest(r.gauss(o, l)) for l in range(nl)] for o in range(no)],
                "dog": [[plane_digest(r.dog(o, l)) for l in range(nl - 1)] for o in range(no)]}
        self.data[k + ".meta"] = np.array(json.dumps(meta))
        self.data.update({"%s.iext%d" % (k, o): r.iext(o).copy() for o in range(no)})
        self.data.update({k + ".features": r.features().copy(), k + ".descriptors": r.descriptors().copy()})
        return r

    def save(self, path):
        np.savez_compressed(path, **self.data)


class RecordedReference:
    """The reference's answers to the calls of one test of tests/test_ref_shim_cpu.py, replayed from
    tests/golden/refshim/<test name>.npz: the same interface as oracle/pyref.py, with every plane replaced by its
    plane_digest."""

    def __init__(self, path):
        self.path = path
        self.z = np.load(path, allow_pickle=False) if os.path.exists(path) else None

    def get(self, k, name):
        f = "%s.%s" % (k, name)
        if self.z is None or f not in self.z.files:
            raise KeyError("%s: no recorded reference answer for this call in %s; re-record with tests/golden/make_refshim.py"
                           % (f, os.path.relpath(self.path, GOLDEN_DIR)))
        return self.z[f]

    def gauss_tables(self, cfg):
        k = _key("tables", cfg)
        names = [f[len(k) + 1:] for f in self.z.files if f.startswith(k + ".")] if self.z is not None else []
        if not names:
            self.get(k, "inc_filter")
        return {n: self.z[k + "." + n] for n in names}

    def match(self, left, right):
        k = _key("match", left, right)
        return self.get(k, "mm"), self.get(k, "dd")

    def run(self, cfg, img, api=False):
        return _RecordedRun(self, _key("run", cfg, img, api))


class _RecordedRun:
    def __init__(self, rec, k):
        self._rec, self._k = rec, k
        m = json.loads(str(rec.get(k, "meta")))
        self.num_octaves, self.num_levels = m["num_octaves"], m["num_levels"]
        self.dims = [tuple(d) for d in m["dims"]]
        self.ext_total, self.ori_total = m["ext_total"], m["ori_total"]
        self._gauss, self._dog = m["gauss"], m["dog"]

    def gauss(self, o, l):
        return self._gauss[o][l]

    def dog(self, o, l):
        return self._dog[o][l]

    def iext(self, o):
        return self._rec.get(self._k, "iext%d" % o)

    def features(self):
        return self._rec.get(self._k, "features")

    def descriptors(self):
        return self._rec.get(self._k, "descriptors")

    def close(self):
        pass
