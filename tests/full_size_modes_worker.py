"""Worker of tests/test_gpu_modes_full_size.py: one process = one setting of the environment switches (they are read at
psx_create).  argv: a JSON file {"cases": [names], "features": bool}, and an output directory.  Writes <case>.npz per case:
the octave dimensions, the digests of every Gaussian plane (tests/full_size_cases.plane_digests), the initial extrema of every
octave and, with "features", the features and descriptors; prints one JSON line of the cases done."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from popsift_amd import capi          # noqa: E402
from tests import full_size_cases as fc  # noqa: E402


def main(spec_path, out_dir):
    spec = json.load(open(spec_path))
    done = []
    for name in spec["cases"]:
        case = fc.BY_NAME[name]
        ctx = capi.Context(capi.default_config(**fc.config(case)))
        ctx.upload(fc.image(case))
        ctx.extract()
        no, nl = ctx.num_octaves, ctx.num_levels
        rec = dict(num_octaves=np.int32(no), num_levels=np.int32(nl),
                   dims=np.array([ctx.octave_dims(o) for o in range(no)], np.int32).reshape(-1, 2))
        for o in range(no):
            for l in range(nl):
                sha, rows, cols = fc.plane_digests(ctx.dump_plane(capi.PLANE_GAUSS, o, l))
                rec["sha_%d_%d" % (o, l)] = np.array(sha)
                rec["rows_%d_%d" % (o, l)] = rows
                rec["cols_%d_%d" % (o, l)] = cols
            ie = ctx.dump_iext(o)
            for f in ("xpos", "ypos", "lpos"):
                rec["iext_%s_%d" % (f, o)] = np.ascontiguousarray(ie[f])
        if spec.get("features"):
            fb, db = ctx.download()
            rec["features"] = fb
            rec["descriptors"] = db
        ctx.close()
        np.savez(os.path.join(out_dir, name + ".npz"), **rec)
        done.append(name)
    print(json.dumps(done))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
