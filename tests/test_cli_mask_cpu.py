"""CPU tests of popsift-demo --mask: the option is on the surface, takes a value, wants an 8-bit grey PGM, and a mask
whose size is not the input's is a clear error with a non-zero exit -- decided from the file headers, before a device is
touched.  (What the option extracts is tests/test_gpu_mask.py's business.)"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "popsift_amd", "lib")


@pytest.fixture(scope="module")
def demo():
    from popsift_amd import build
    build.build_all()
    return os.path.join(LIB, "popsift-demo")


def write_pgm(path, a):
    path.write_bytes(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + np.ascontiguousarray(a, np.uint8).tobytes())


def run(demo, argv, cwd):
    return subprocess.run([demo] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(cwd), timeout=120)


def test_mask_option_on_the_surface(demo):
    p = subprocess.run([demo, "--help"], stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "--mask arg" in p.stdout


def test_mask_option_rejects_bad_command_lines(demo, tmp_path):
    rng = np.random.default_rng(3)
    write_pgm(tmp_path / "a.pgm", rng.integers(0, 256, (48, 64)))
    write_pgm(tmp_path / "m_ok.pgm", np.ones((48, 64)))
    write_pgm(tmp_path / "m_small.pgm", np.ones((48, 63)))
    (tmp_path / "m_colour.ppm").write_bytes(b"P6\n64 48\n255\n" + bytes(64 * 48 * 3))
    (tmp_path / "m_16bit.pgm").write_bytes(b"P5\n64 48\n999\n" + bytes(64 * 48 * 2))
    (tmp_path / "m_short.pgm").write_bytes(b"P5\n64 48\n255\n" + bytes(100))
    # no value; an empty value
    assert run(demo, ["-i", "a.pgm", "--mask"], tmp_path).returncode != 0
    assert run(demo, ["-i", "a.pgm", "--mask="], tmp_path).returncode != 0
    # a file that is not there, not grey, not 8 bit, too short
    for m, word in (("missing.pgm", "not a readable PGM"), ("m_colour.ppm", "8-bit grey"), ("m_16bit.pgm", "8-bit grey"), ("m_short.pgm", "too short")):
        p = run(demo, ["-i", "a.pgm", "--mask", m], tmp_path)
        assert p.returncode != 0 and word in p.stderr, (m, p.stderr)
    # another size: both sizes named, no output file
    p = run(demo, ["-i", "a.pgm", "--mask", "m_small.pgm"], tmp_path)
    assert p.returncode != 0 and "63 x 48" in p.stderr and "64 x 48" in p.stderr, p.stderr
    assert not (tmp_path / "output-features.txt").exists()
    # a directory with one image of another size
    d = tmp_path / "dir"
    d.mkdir()
    write_pgm(d / "a.pgm", rng.integers(0, 256, (48, 64)))
    write_pgm(d / "b.pgm", rng.integers(0, 256, (40, 64)))
    p = run(demo, ["-i", "dir", "--mask=m_ok.pgm"], tmp_path)
    assert p.returncode != 0 and "64 x 40" in p.stderr and "b.pgm" in p.stderr, p.stderr
