"""The host steps of FeaturesDev's matching, RANSAC and track wrappers (popsift_amd/csrc/host/features.cpp) without a device.

tests/cpp/features_wrappers_san.cpp is a stand-alone program: features.cpp compiled together with stubs of the 36 psx_*
functions it reaches the device through, under -fsanitize=address,undefined.  It logs every device-work call of every public
wrapper -- allocation sizes, what is quantised and gathered for which view, the final call with every argument -- prints the
returned fields, and then makes each device-work call of five wrappers fail in turn.  The transcript is this
project's own output, recorded once and kept in tests/golden/features_wrappers_transcript.txt: which entry point a wrapper
calls, with which arguments, after which preparation, and what it returns must not change."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "features_wrappers_transcript.txt")
# the failure-injection cases the program must run: wrapper -> its device-work calls
INJECTED = {"FeaturesDev::matchPairsGuidedGraph": 13, "FeaturesDev::matchPairsGuidedMany": 13, "FeaturesDev::estimateHomographyGraph": 7,
            "FeaturesDev::matchPairsGuided": 9, "FeaturesDev::estimateAffineMany": 7}


@pytest.fixture(scope="module")
def transcript(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path_factory.mktemp("features_wrappers") / "features_wrappers_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "features_wrappers_san.cpp"),
           os.path.join(ROOT, "popsift_amd", "csrc", "host", "features.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "popsift_amd", "csrc", "host"),
           "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "FEATURES_WRAPPERS_READS"}
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)


def test_wrappers_under_sanitizers(transcript):
    """a clean exit: no sanitizer report, no harness check failed, every device buffer freed"""
    assert transcript.returncode == 0 and transcript.stderr == b"", transcript.stderr.decode(errors="replace")[-4000:]
    assert transcript.stdout.endswith(b"ALL OK\n"), transcript.stdout.decode(errors="replace")[-2000:]


def test_transcript_equals_golden(transcript):
    """every device-work call, every argument, every returned field and every message, byte for byte"""
    with open(GOLDEN, "rb") as f:
        golden = f.read()
    if transcript.stdout != golden:
        got, want = transcript.stdout.decode(errors="replace").splitlines(), golden.decode().splitlines()
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        head = next((l for l in reversed(want[:at + 1]) if l.startswith("== ")), "")
        pytest.fail("transcript differs from the golden file at line %d (%s):\n  got:  %s\n  want: %s"
                    % (at + 1, head, got[at] if at < len(got) else "<end>", want[at] if at < len(want) else "<end>"))


def test_failure_injection(transcript):
    """each device-work call of the guided byte edge-list form, the guided byte star and estimateGraph (and of one single form
    and one RANSAC star) failed once: a preparation call with a code other than PSX_ERR_INVALID, the final call with
    PSX_ERR_INVALID.  Every time the wrapper threw "<name> failed"; the program itself checks that the live device
    allocations and bytes returned to their value before the call, and aborts otherwise."""
    assert transcript.returncode == 0
    lines = transcript.stdout.decode().splitlines()
    seen = {}
    for i, line in enumerate(lines):
        m = re.match(r"== inject (\S+): (\d+) device-work calls$", line)
        if not m:
            continue
        name, n = m.group(1), int(m.group(2))
        seen[name] = n
        body = lines[i + 1:i + 1 + n]
        assert len(body) == n and [b.split(":")[0] for b in body] == [" n=%d" % k for k in range(1, n + 1)], body
        for b in body[:-1]:
            assert b.endswith("features.cpp:N %s failed (-2)" % name), b
        assert ("features.cpp:N %s failed (-1: invalid options" % name) in body[-1], body[-1]
    assert seen == INJECTED
