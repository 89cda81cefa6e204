"""GPU tests of byte descriptors through the C++ layers: PopSift / SiftJob / FeaturesHost with
Config::ByteDescriptors (DMA result path, POPSIFT_EXPORT=1 zero-copy export, the pageable fallback beyond
POPSIFT_PINNED_LIMIT_MB), the flat C binding behind capi.PopSift, and the --uchar-descriptors flags of popsift-demo
and popsift-match."""
import os
import subprocess
import sys

import numpy as np
import pytest

from popsift_amd import capi
from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "popsift_amd", "lib", "popsift-demo")
MATCH = os.path.join(ROOT, "popsift_amd", "lib", "popsift-match")


def _rows(feats, desc):
    """canonical order: one row per (keypoint, orientation) keyed by its record, with its descriptor row"""
    keys, rows = [], []
    for f in feats:
        for k in range(f["num_ori"]):
            keys.append(np.array([f["xpos"], f["ypos"], f["sigma"], f["orientation"][k]], np.float32).tobytes())
            rows.append(desc[f["desc_idx"][k]])
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    return [keys[i] for i in order], np.array([rows[i] for i in order]).reshape(-1, 128)


@pytest.mark.parametrize("env", ["dma", "export", "hoarding"])
def test_popsift_byte_mode_equals_rule_of_float_mode(tmp_path, env):
    """1080p VLFeat frames with 24 jobs outstanding through PopSift in float and in byte mode: per frame the same records
    (canonical order) and bytes == rule(floats); the pinned pool stays flat over a second pass of the same PopSift and is
    empty after close()."""
    e = dict(os.environ)
    if env == "export":
        e["POPSIFT_EXPORT"] = "1"
    if env == "hoarding":
        e["POPSIFT_PINNED_LIMIT_MB"] = "0"
    out = str(tmp_path / "r.npz")
    n = 30
    subprocess.run([sys.executable, "-m", "tests.byte_popsift_worker", out, str(n), "24", "1920", "1080"], cwd=ROOT, env=e,
                   check=True, timeout=600)
    z = np.load(out)
    for i in range(n):
        ff, df = z["f32_feat_%d" % i], z["f32_desc_%d" % i]
        fb, db = z["u8_feat_%d" % i], z["u8_desc_%d" % i]
        assert db.dtype == np.uint8 and df.dtype == np.float32
        assert len(ff) == len(fb) and len(df) == len(db) and len(db) > 1000
        kf, rf = _rows(ff, df)
        kb, rb = _rows(fb, db)
        assert kf == kb
        assert np.array_equal(rb, capi.quantize_rule(rf))
    for name in ("f32", "u8"):
        warm, after, in_use = z["%s_pool" % name]
        # steady stream: no allocation beyond a new high-water mark of simultaneously live buffers (the workers and the
        # caller race for buffers: the peak can move by a buffer or two between passes -- the tolerance of
        # tests/test_gpu_headline.py's pool test)
        assert after - warm <= 3, (name, warm, after)
        assert in_use == 0, (name, in_use)


def test_flat_c_copy_refuses_floats_of_a_byte_result():
    H = capi.host_lib()
    ps = capi.PopSift(capi.default_config(octaves=3), byte_descriptors=True)
    job = ps.enqueue(synth(320, 240, 5))
    f = H.popsift_c_get(job)
    assert f
    try:
        no = H.popsift_c_descriptor_count(f)
        assert no > 0 and H.popsift_c_descriptor_format(f) == capi.DESCFMT_U8
        assert H.popsift_c_descriptors(f) is None and H.popsift_c_descriptor_bytes(f)
        buf = np.zeros((no, 128), np.float32)
        assert H.popsift_c_copy(f, None, buf.ctypes.data) == -4            # PSX_ERR_STATE
        assert b"byte descriptors" in H.popsift_c_last_error()
        assert H.popsift_c_copy(f, None, None) == 0
    finally:
        H.popsift_c_free(f)
        ps.close()


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def _run(cmd, cwd):
    p = subprocess.run(cmd, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def test_demo_uchar_descriptors_equals_write_as_uchar(tmp_path):
    """popsift-demo --norm-multi 9 --uchar-descriptors writes the lines of --write-as-uchar in float mode (sorted): with
    Classic normalisation no value exceeds 255, so the saturation never differs from the reference's text."""
    img = synth(400, 300, 88)
    _write_pgm(tmp_path / "a.pgm", img)
    common = [DEMO, "-i", "a.pgm", "--octaves", "3", "--norm-multi", "9", "--norm-mode", "classic"]
    _run(common + ["--write-as-uchar"], tmp_path)
    a = np.loadtxt(str(tmp_path / "output-features.txt"), ndmin=2)
    _run(common + ["--uchar-descriptors"], tmp_path)
    b = np.loadtxt(str(tmp_path / "output-features.txt"), ndmin=2)
    assert a.shape == b.shape and len(a) > 50
    assert a[:, 5:].max() <= 255
    srt = lambda m: m[np.lexsort(m.T[::-1])]
    assert np.array_equal(srt(a), srt(b))


def test_match_uchar_descriptors(oracle, tmp_path):
    base = synth(336, 256, 77)
    a = np.ascontiguousarray(base[8:248, 8:328])
    b = np.ascontiguousarray(base[5:245, 3:323])
    _write_pgm(tmp_path / "l.pgm", a)
    _write_pgm(tmp_path / "r.pgm", b)
    args = [MATCH, "-l", "l.pgm", "-r", "r.pgm", "--octaves", "3", "--norm-multi", "9"]
    pf = _run(args, tmp_path)
    pb = _run(args + ["--uchar-descriptors"], tmp_path)
    lf = [l for l in pf.stdout.splitlines() if l.startswith(("accept", "reject"))]
    lb = [l for l in pb.stdout.splitlines() if l.startswith(("accept", "reject"))]
    assert len(lf) == len(lb) > 50
    # the same extraction through the C-ABI, quantised, matched by the oracle: the same accept / reject per descriptor
    ds = []
    for img in (a, b):
        ctx = capi.Context(capi.default_config(octaves=3, norm_multi=9))
        ctx.upload(img)
        ctx.extract()
        ds.append(capi.quantize_rule(ctx.download()[1]))
        ctx.close()
    mo, _ = oracle.match(ds[0].astype(np.float32), ds[1].astype(np.float32))
    acc_b = sum(l.startswith("accept") for l in lb)
    assert acc_b == int(mo[:, 2].sum())
    assert acc_b > 0.3 * len(lb)
