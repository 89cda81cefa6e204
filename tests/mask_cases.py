"""Shared by tests/test_mask_cpu.py, tests/test_gpu_mask.py and tests/mask_popsift_worker.py: the detection masks the
tests use, the configurations they run on, and the rule of include/popsift_hip.h ("detection mask") restated in numpy."""
import numpy as np

from tests.test_keypoints_cpu import ROUND_TRIP

# keyword arguments of default_config, image size, synth seed
FULL_HD = (dict(sift_mode=2), (1920, 1080), 1000)
CONFIGS = ROUND_TRIP + [FULL_HD]
CONFIG_IDS = ["640x480-default", "640x480-vlfeat", "480x360-levels4", "800x600-opencv-down", "1920x1080-vlfeat"]

MASKS = ("half", "checker1", "disc", "blocks16")


def make_mask(name, w, h, seed=7):
    """(h, w) uint8; non-zero = keypoints allowed"""
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "half":
        return np.where(xx < w // 2, 255, 0).astype(np.uint8)
    if name == "checker1":                 # cells of one pixel, values 0 / 1: any slip in the rounding shows at once
        return ((xx + yy) & 1).astype(np.uint8)
    if name == "disc":
        r = 0.45 * min(w, h)
        inside = (xx - w / 2.0) ** 2 + (yy - h / 2.0) ** 2 <= r * r
        return np.where(inside, 7, 0).astype(np.uint8)
    if name == "blocks16":                 # 16 x 16 blocks of values 0..3: "non-zero" is not "255"
        cells = np.random.default_rng(seed).integers(0, 4, ((h + 15) // 16, (w + 15) // 16), dtype=np.uint8)
        return np.ascontiguousarray(np.kron(cells, np.ones((16, 16), np.uint8))[:h, :w])
    if name == "ones":
        return np.ones((h, w), np.uint8)
    if name == "zeros":
        return np.zeros((h, w), np.uint8)
    raise KeyError(name)


def pixel(v, n):
    """clamp((int)floorf(v + 0.5f), 0, n - 1) in float32 arithmetic: the sum is rounded to float32 before the floor"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(v, np.float32) + np.float32(0.5))
    f = np.where(np.isnan(f), 0.0, f)
    return np.clip(f, 0, n - 1).astype(np.int64)


def restate_keep(mask, xpos, ypos):
    """the rule on reported positions: bool array, True = allowed"""
    h, w = mask.shape
    return mask[pixel(ypos, h), pixel(xpos, w)] != 0


def assert_premise(name, kept, total, what=""):
    """Both outcomes of the rule are exercised by hundreds of keypoints: more than 300 kept and more than 300 rejected.
    blocks16 clears one block value in four by construction, so on a configuration with fewer than ~1200 keypoints it
    cannot reject 300 (about 160 of the 628 on the downsampled OpenCV frame): there the bar for the
    rejected side is a fifth of the keypoints -- the expected quarter less a margin for where the keypoints lie."""
    rejected = total - kept
    need_rejected = min(300, total // 5) if name == "blocks16" else 300
    assert kept > 300 and rejected > need_rejected, (what, name, kept, rejected, total)
