"""The environment switches of libpopsift_hip.so without a GPU: popsift_amd/csrc/hip/psx_tuning.h, compiled for the host.

One table, one struct, one parser: tests/cpp/tuning_shim.cpp wraps the header, this file sets the environment, lets the
parser walk the table and reads the field back.  The expected values below are what the code accepted before the table
existed (one getenv() per switch, spread over seven files): for every row the default with the variable unset, an
accepted non-default value, the nearest rejected value on each side of the range (or outside the set), and by name the
switches whose rule is their own.  The source checks at the end keep the table the only reader of the environment.
"""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "popsift_amd", "csrc", "hip")

# every name getenv() was called with under popsift_amd/csrc/hip before the table existed
NAMES = """
POPSIFT_ALT_WGS POPSIFT_ALT_WINDOW POPSIFT_BATCH_OCTAVES POPSIFT_BLUR_DBG POPSIFT_BLUR_DEFER POPSIFT_BLUR_DMA
POPSIFT_BLUR_DMA_STEPS POPSIFT_BLUR_LDS_PAD POPSIFT_BLUR_ONESTEP POPSIFT_BLUR_STEPS POPSIFT_CU_PARTITIONS
POPSIFT_CU_PARTITION_MODE POPSIFT_DESC_DENORM POPSIFT_DESC_OCC POPSIFT_DESC_WGS POPSIFT_DESC_WPB POPSIFT_FIXED_FUSED
POPSIFT_FIXED_MINSTEPS POPSIFT_FIXED_WGS POPSIFT_FLOW POPSIFT_FLOW_DEBUG POPSIFT_FLOW_GRID POPSIFT_FLOW_LD
POPSIFT_FLOW_ORDER POPSIFT_FLOW_STEPS POPSIFT_HIP_GRAPH POPSIFT_INTERP_DIAGONAL POPSIFT_INTERP_FUSED
POPSIFT_INTERP_LITERAL POPSIFT_INTERP_MINWG POPSIFT_INTERP_ONESTEP POPSIFT_INTERP_PAIR_ROUNDS POPSIFT_INTERP_STEPS
POPSIFT_LEVEL0_FUSED POPSIFT_LEVEL0_X2 POPSIFT_MATCH_MFMA POPSIFT_MATCH_ROUNDS POPSIFT_MATCH_STATS
POPSIFT_MATCH_WGS_PER_CU POPSIFT_ORI_WPB POPSIFT_TILE POPSIFT_TILE_MAXPX POPSIFT_TILE_NT POPSIFT_TILE_SMALL
POPSIFT_TILE_TY POPSIFT_WAIT_SLEEP_US PSX_NULL_DEVICE_WORK
""".split()

FLOW_TEXT = ": valid values are 0 (one launch per level), 1 (every level in one launch), 2 (octave 0 by launches)"

ON = (1, {"0": 0, "0x": 0, "1": 1, "": 1, "off": 1})          # off only when the value starts with '0'
OFF = (0, {"1": 1, "1x": 1, "0": 0, "2": 0, "": 0, "on": 0})    # on only when the value starts with '1'

# name -> (default, {value: what the field holds afterwards})
CASES = {
    "POPSIFT_LEVEL0_FUSED": ON, "POPSIFT_LEVEL0_X2": ON, "POPSIFT_BATCH_OCTAVES": ON, "POPSIFT_MATCH_MFMA": ON,
    "POPSIFT_DESC_DENORM": ON, "POPSIFT_INTERP_ONESTEP": ON, "POPSIFT_INTERP_DIAGONAL": ON, "POPSIFT_TILE_SMALL": ON,
    "POPSIFT_ALT_WINDOW": ON, "POPSIFT_FIXED_FUSED": ON, "POPSIFT_INTERP_FUSED": ON, "POPSIFT_BLUR_DEFER": ON,
    "POPSIFT_HIP_GRAPH": OFF, "POPSIFT_BLUR_ONESTEP": OFF, "POPSIFT_INTERP_LITERAL": OFF,
    # integer in a range
    "POPSIFT_BLUR_STEPS": (5, {"7": 7, "2": 2, "64": 64, "1": 5, "65": 5}),
    "POPSIFT_BLUR_DMA_STEPS": (0, {"6": 6, "2": 2, "64": 64, "1": 0, "65": 0}),
    "POPSIFT_BLUR_DMA": (0, {"2": 2, "3": 3, "-1": 0, "4": 0}),
    "POPSIFT_INTERP_STEPS": (5, {"3": 3, "2": 2, "64": 64, "1": 5, "65": 5}),
    "POPSIFT_INTERP_MINWG": (384, {"256": 256, "1": 1, "0": 384, "-1": 384}),
    "POPSIFT_INTERP_PAIR_ROUNDS": (100, {"150": 150, "50": 50, "1000": 1000, "49": 100, "1001": 100}),
    "POPSIFT_FIXED_MINSTEPS": (1, {"2": 2, "8": 8, "0": 1, "9": 1}),
    "POPSIFT_DESC_WGS": (0, {"10": 10, "1": 1, "64": 64, "0": 0, "-1": 0, "65": 0}),
    "POPSIFT_ALT_WGS": (8, {"4": 4, "1": 1, "64": 64, "0": 8, "65": 8}),
    "POPSIFT_MATCH_ROUNDS": (1, {"2": 2, "4": 4, "0": 1, "5": 1}),
    "POPSIFT_MATCH_WGS_PER_CU": (0, {"3": 3, "1": 1, "8": 8, "0": 0, "9": 0}),
    "POPSIFT_CU_PARTITIONS": (0, {"4": 4, "2": 2, "8": 8, "1": 0, "9": 0}),
    "POPSIFT_FLOW_GRID": (0, {"64": 64, "8": 8, "7": 0, "-8": 0}),
    # integer from a set
    "POPSIFT_TILE_TY": (64, {"32": 32, "8": 8, "128": 128, "30": 64, "4": 64, "132": 64}),
    "POPSIFT_TILE_NT": (1024, {"512": 512, "1024": 1024, "256": 1024, "768": 1024, "2048": 1024}),
    "POPSIFT_DESC_WPB": (0, {"1": 1, "2": 2, "4": 4, "3": 0, "8": 0}),
    "POPSIFT_ORI_WPB": (4, {"1": 1, "4": 4, "2": 4, "0": 4, "8": 4}),
    # one digit, the first character decides
    "POPSIFT_TILE": (0, {"1": 1, "1x": 1, "0": 0, "2": 0, "": 0}),
    "POPSIFT_FLOW_LD": (2, {"1": 1, "2": 2, "0": 2, "3": 2}),
    "POPSIFT_FLOW_ORDER": (0, {"2": 2, "1": 1, "3": 0, "-1": 0}),
    "PSX_NULL_DEVICE_WORK": (0, {"1": 1, "2": 2, "0": 0, "3": 0}),
    "POPSIFT_DESC_OCC": (0, {"5": 5, "4": 0, "6": 0}),
    # rules of their own
    "POPSIFT_MATCH_STATS": (0, {"1": 1, "0": 1, "": 1}),                      # on when set to anything
    "POPSIFT_WAIT_SLEEP_US": (40, {"100": 100, "0": 0, "-5": 0}),             # a negative value means 0, not 40
    "POPSIFT_TILE_MAXPX": (3 << 20, {"1000000": 1000000, "0": 0, "8589934592": 8589934592, "-1": 3 << 20}),
    "POPSIFT_BLUR_LDS_PAD": (0, {"4096": 4096}),                              # unchecked atoi from here on
    "POPSIFT_FIXED_WGS": (0, {"512": 512, "-5": -5}),
    "POPSIFT_CU_PARTITION_MODE": (0, {"1": 1, "7": 7}),
    "POPSIFT_FLOW_DEBUG": (0, {"2": 2, "9": 9}),
    "POPSIFT_BLUR_DBG": (0, {"3": 3}),
    "POPSIFT_FLOW_STEPS": ("3,2,1", {"5,0": "5,0", "": ""}),                  # a comma list, parsed by the planner
    "POPSIFT_FLOW": (0, {"1": 1, "2": 2, "0": 0, "": 0}),                     # strict: see test_flow_is_strict
}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    so = str(tmp_path_factory.mktemp("tuning") / "libtuning_shim.so")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", HIP,
                           os.path.join(ROOT, "tests", "cpp", "tuning_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.tuning_get.restype = C.c_int
    lib.tuning_get.argtypes = [C.c_char_p, C.POINTER(C.c_longlong), C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.tuning_rows.restype = C.c_int
    lib.tuning_rows.argtypes = [C.c_char_p, C.c_int]
    return lib


@pytest.fixture
def clean_env(monkeypatch):
    for n in NAMES:
        monkeypatch.delenv(n, raising=False)
    return monkeypatch


def get(shim, name):
    """(field as int or str, error text) after one walk of the table"""
    v = C.c_longlong(0)
    text, err = C.create_string_buffer(256), C.create_string_buffer(512)
    assert shim.tuning_get(name.encode(), C.byref(v), text, 256, err, 512) == 0, "no row for " + name
    return (text.value.decode() if name == "POPSIFT_FLOW_STEPS" else v.value), err.value.decode()


def rows(shim):
    buf = C.create_string_buffer(1 << 14)
    assert shim.tuning_rows(buf, 1 << 14) < (1 << 14)
    return [ln.split(" ", 2) for ln in buf.value.decode().splitlines()]


def test_every_row_has_cases():
    assert sorted(CASES) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_row(shim, clean_env, name):
    default, values = CASES[name]
    assert get(shim, name) == (default, "")
    assert any(want != default for want in values.values()), "no accepted non-default value"
    for value, want in values.items():
        clean_env.setenv(name, value)
        assert get(shim, name) == (want, ""), "%s=%r" % (name, value)
        for other in NAMES:                          # a switch moves its own field only
            if other != name:
                assert get(shim, other)[0] == CASES[other][0], "%s=%r changed %s" % (name, value, other)
        clean_env.delenv(name)


def test_oddities_by_name(shim, clean_env):
    for name, value, want in (("POPSIFT_MATCH_STATS", "0", 1), ("POPSIFT_BLUR_DEFER", "", 1), ("POPSIFT_TILE_TY", "30", 64),
                              ("POPSIFT_HIP_GRAPH", "2", 0), ("POPSIFT_DESC_OCC", "5", 5), ("POPSIFT_DESC_OCC", "4", 0),
                              ("POPSIFT_WAIT_SLEEP_US", "-1", 0), ("POPSIFT_TILE_MAXPX", "-1", 3 << 20)):
        clean_env.setenv(name, value)
        assert get(shim, name) == (want, ""), "%s=%r" % (name, value)
        clean_env.delenv(name)


def test_flow_is_strict(shim, clean_env):
    """anything but 0, 1, 2 (and the empty string) is an error with the text psx_create has always failed with"""
    for bad in ("3", "01", "1 ", "on", "-1"):
        clean_env.setenv("POPSIFT_FLOW", bad)
        value, err = get(shim, "POPSIFT_FLOW")
        assert value == 0 and err == "POPSIFT_FLOW=" + bad + FLOW_TEXT
    clean_env.setenv("POPSIFT_FLOW", "2")
    assert get(shim, "POPSIFT_FLOW") == (2, "")
    # no other row is strict: a bad value elsewhere is the default, silently
    clean_env.setenv("POPSIFT_FLOW_LD", "7")
    assert get(shim, "POPSIFT_FLOW_LD") == (2, "")


def test_table_names_and_defaults(shim, clean_env):
    r = rows(shim)
    assert sorted(n for n, _, _ in r) == sorted(NAMES)           # one row per name, no new name
    for n, kind, default in r:
        assert str(CASES[n][0]) == default, n
        assert kind in ("ON", "OFF", "SET", "INT", "LL", "DIGIT", "STR", "STRICT")
    assert [n for n, kind, _ in r if kind == "STRICT"] == ["POPSIFT_FLOW"]


def sources():
    return sorted(glob.glob(os.path.join(HIP, "*")))


def test_one_reader_of_the_environment():
    readers = [os.path.basename(f) for f in sources() if "getenv" in open(f).read()]
    assert readers == ["psx_tuning.h"]
    header = open(os.path.join(HIP, "psx_tuning.h")).read()
    assert "hip_runtime" not in header and "psx_internal" not in header          # host only


def test_no_device_facts_cached_per_process():
    for f in sources():
        assert "device_cus" not in open(f).read(), f
    # no function-local static that holds an environment value or a device property
    for f in sources():
        for ln in open(f).read().splitlines():
            assert not re.search(r"static const \w+ \w+ = \[\]", ln), "%s: %s" % (f, ln.strip())


def test_integration_md_lists_the_table():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert len(re.findall(r"^\| `%s` \|" % n, doc, re.M)) == 1, "INTEGRATION.md: one row for " + n
    section = doc[doc.index("## 7. Environment switches"):]
    named = set(re.findall(r"\bPOPSIFT_[A-Z0-9_]+\b", doc)) | set(re.findall(r"\bPSX_[A-Z0-9_]+\b", section))
    known = set(NAMES)
    for f in glob.glob(os.path.join(ROOT, "popsift_amd", "csrc", "host", "**", "*"), recursive=True) + \
            glob.glob(os.path.join(ROOT, "popsift_amd", "*.py")):
        if os.path.isfile(f):
            known |= set(re.findall(r"\b(?:POPSIFT|PSX)_[A-Z0-9_]+\b", open(f, errors="replace").read()))
    assert named <= known, sorted(named - known)


def test_integration_md_defaults(shim):
    """the Default column of a HIP-library row is the table's default"""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n, kind, default in rows(shim):
        cell = re.search(r"^\| `%s` \| ([^|]*) \|" % n, doc, re.M).group(1).strip()
        want = {"True": "1", "False": "0"}.get(default, default)
        if kind in ("ON", "OFF", "SET"):
            want = "1" if default == "1" else ("unset" if kind == "SET" else "0")
        assert cell.split(" ")[0].strip("`\"") == want, "%s: INTEGRATION.md says %r, the table %r" % (n, cell, want)
