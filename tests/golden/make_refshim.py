#!/usr/bin/env python3
"""Record tests/golden/refshim/<test name>.npz: the reference's own answers to every call tests/test_ref_shim_cpu.py makes.

Runs that module against the live reference (oracle/_ref/libpopsift_ref.so, the reference's sources compiled for the
CPU through the CUDA emulation in oracle/ref_shim; `make -C oracle ref` where the sources are, REF_SRC=<path>) with
OSIFT_REFSHIM_RECORD set: every oracle-vs-reference assertion is checked live while the answers are recorded.
    make -C oracle ref && python tests/golden/make_refshim.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import pyref
    if not pyref.available():
        sys.exit("oracle/_ref/libpopsift_ref.so is not built (make -C oracle ref)")
    out = os.path.join(ROOT, "tests", "golden", "refshim")
    rc = subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_ref_shim_cpu.py"],
                         cwd=ROOT, env=dict(os.environ, OSIFT_REFSHIM_RECORD=out))
    if rc == 0:
        for f in sorted(os.listdir(out)):
            print("wrote %s (%d bytes)" % (os.path.join(out, f), os.path.getsize(os.path.join(out, f))))
    sys.exit(rc)
