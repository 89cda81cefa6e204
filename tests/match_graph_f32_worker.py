"""Child process of tests/test_gpu_match_graph_f32.py: psx_match_pairs_graph on the BIG case of
tests/match_graph_f32_cases.py in both flavours, under whatever POPSIFT_MATCH_MFMA the parent set.  Prints one JSON line:
for every (flavour, ratio, mutual) the path the call took, whether it fell back, and the SHA-1 of the records and counts."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from popsift_amd import capi                                                              # noqa: E402
from tests.match_graph_f32_cases import BIG_EDGES, BIG_LENS, BIG_SEED, FLAVOURS, graph_sets_f32    # noqa: E402

WORKER_COMBOS = ((0.8, True), (0.8, False), (float("inf"), True))


def digest(records, counts):
    return hashlib.sha1(records.tobytes() + np.asarray(counts).astype("<i4").tobytes()).hexdigest()


def main():
    out = {}
    for which in FLAVOURS:
        sets = graph_sets_f32(BIG_SEED, BIG_LENS, which)
        for ratio, mutual in WORKER_COMBOS:
            lists, counts = capi.match_pairs_graph(sets, BIG_EDGES, ratio, mutual)
            info = capi.match_graph_f32_last()
            rec = np.concatenate(lists) if lists else np.zeros(0, capi.PAIR_DTYPE)
            out["%s/%r/%d" % (which, ratio, mutual)] = [info["path"], info["fell_back"], digest(rec, counts)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
