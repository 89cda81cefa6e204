"""Child process of tests/test_gpu_match_many_f32.py: psx_match_pairs_many on the planted cases of the seeds given on the
command line, in both flavours, under whatever POPSIFT_MATCH_MFMA the parent set.  Prints one JSON line: for every
(seed, flavour, ratio, mutual) the path the call took, whether it fell back, and the SHA-1 of the records and counts."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from popsift_amd import capi                                                      # noqa: E402
from tests.match_many_f32_cases import CASES, FLAVOURS, planted_many_f32          # noqa: E402

WORKER_COMBOS = ((0.8, True), (0.8, False), (float("inf"), True))


def digest(records, counts):
    return hashlib.sha1(records.tobytes() + counts.astype("<i4").tobytes()).hexdigest()


def main():
    out = {}
    for seed in [int(a) for a in sys.argv[1:]]:
        _, nl, lens = [c for c in CASES if c[0] == seed][0]
        for which in FLAVOURS:
            left, rights = planted_many_f32(seed, nl, lens, which)
            for ratio, mutual in WORKER_COMBOS:
                lists, counts = capi.match_pairs_many(left, rights, ratio, mutual)
                info = capi.match_many_f32_last()
                rec = np.concatenate(lists) if lists else np.zeros(0, capi.PAIR_DTYPE)
                out["%d/%s/%r/%d" % (seed, which, ratio, mutual)] = [info["path"], info["fell_back"], digest(rec, counts)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
