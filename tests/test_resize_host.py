"""CPU tests of the Pillow-exact resize (the demo's per-request steps, demo.py:39-73): the Python restatement
(tests/pil_resample_util.py) against the installed Pillow, the library's host-side coefficient tables
(se_resample_coeffs) against the restatement, the C-ABI declarations, and serve.py's device-path request decoding."""
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image

import pil_resample_util as R
from sketchedit_amd import _lib, serve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = [R.BICUBIC, R.BILINEAR, R.LANCZOS]
# (w_in, h_in) -> (w_out, h_out): identity, identity on one axis, the demo's /8 flooring, x5 down, x3 up, 1-pixel
# dimensions, a 250-tap downscale
SWEEP = [((70, 67), (70, 67)), ((70, 67), (70, 64)), ((70, 67), (64, 67)), ((641, 481), (640, 480)), ((70, 67), (64, 64)),
         ((320, 160), (64, 32)), ((40, 24), (120, 72)), ((1, 9), (5, 1)), ((7, 1), (1, 3)), ((999, 5), (16, 16)),
         ((300, 17), (37, 160)), ((33, 33), (33, 40))]


@pytest.fixture(scope="module")
def built_lib():
    _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.se_resample_coeffs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.se_resample_coeffs.restype = ctypes.c_int
    return lib


def lib_coeffs(lib, n_in, n_out, filt):
    ksize = lib.se_resample_coeffs(n_in, n_out, filt, None, None, 0)
    assert ksize > 0
    bounds = np.zeros((n_out, 2), np.int32)
    k = np.zeros((n_out, ksize), np.int32)
    assert lib.se_resample_coeffs(n_in, n_out, filt, bounds.ctypes.data, k.ctypes.data, k.size) == ksize
    return bounds, k


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_restatement_is_pillow(filt, mode):
    rng = np.random.RandomState(filt * 7 + len(mode))
    for (wi, hi), (wo, ho) in SWEEP:
        a = rng.randint(0, 256, (hi, wi, 3) if mode == "RGB" else (hi, wi)).astype(np.uint8)
        ref = np.asarray(Image.fromarray(a, mode).resize((wo, ho), filt))
        assert np.array_equal(R.resize(a, (wo, ho), filt), ref), ((wi, hi), (wo, ho))


def test_restatement_rings_like_pillow_on_a_sparse_sketch():
    """The sketch's `> 0` after a bicubic resize is decided by ringing around thin lines: the restatement keeps every
    pixel Pillow lets into the mask, and no other."""
    rng = np.random.RandomState(5)
    sk = ((rng.rand(481, 641) < 0.01) * 255).astype(np.uint8)
    ref = np.asarray(Image.fromarray(sk).resize((640, 480))) > 0
    got = R.resize(sk, (640, 480)) > 0
    assert np.array_equal(got, ref) and 0 < ref.sum() < ref.size


def test_restatement_copies_a_photo_sized_identity():
    a = np.random.RandomState(1).randint(0, 256, (3024, 4032, 3)).astype(np.uint8)
    got = R.resize(a, (4032, 3024))
    assert np.array_equal(got, np.asarray(Image.fromarray(a).resize((4032, 3024)))) and got is not a


@pytest.mark.parametrize("filt", FILTERS)
def test_library_coefficients_are_the_restatements(built_lib, filt):
    sizes = {(i, o) for (wi, hi), (wo, ho) in SWEEP for i, o in ((wi, wo), (hi, ho))} | {(4032, 4032), (1081, 1080), (1920, 1921)}
    for n_in, n_out in sorted(sizes):
        bounds, k = lib_coeffs(built_lib, n_in, n_out, filt)
        rb, rk = R.coeffs(n_in, n_out, filt)
        assert np.array_equal(bounds, rb), (n_in, n_out)
        assert np.array_equal(k, rk), (n_in, n_out)


def test_library_coefficients_refuse_bad_arguments(built_lib):
    assert built_lib.se_resample_coeffs(10, 0, R.BICUBIC, None, None, 0) < 0
    assert built_lib.se_resample_coeffs(0, 10, R.BICUBIC, None, None, 0) < 0
    assert built_lib.se_resample_coeffs(10, 10, 0, None, None, 0) < 0        # NEAREST is not a separable filter here
    assert built_lib.se_resample_coeffs(999, 16, R.BICUBIC, None, None, 0) == 251


def test_header_declares_the_resize_entries():
    hdr = open(os.path.join(ROOT, "include", "sketchedit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in ("se_resize_u8", "se_prepare_u8", "se_edit_u8", "se_edit_u8_workspace_bytes", "se_resample_coeffs"):
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert s in _lib.abi_names("sketchedit_hip.h"), s
    consts = dict(re.findall(r"SE_RESAMPLE_(\w+)\s*=\s*(\d+)", code))
    assert {k: int(v) for k, v in consts.items()} == {"LANCZOS": int(Image.Resampling.LANCZOS),
                                                        "BILINEAR": int(Image.Resampling.BILINEAR),
                                                        "BICUBIC": int(Image.Resampling.BICUBIC)}
    assert (_lib.RESAMPLE_LANCZOS, _lib.RESAMPLE_BILINEAR, _lib.RESAMPLE_BICUBIC) == (1, 2, 3)


def test_device_inputs_of_a_request():
    """serve._device_inputs: RGB uint8 image; the sketch plane as is for 'L', channel 0 for 'RGB' (Pillow resamples
    channels independently, so the host path's `[..., 0]` after the resize is the resize of that plane); None (host
    preparation) for the modes Pillow resamples differently; too small a request raises as _to_tensors does."""
    rng = np.random.RandomState(2)
    img = Image.fromarray(rng.randint(0, 256, (67, 70, 3)).astype(np.uint8))
    sk = rng.randint(0, 256, (50, 41)).astype(np.uint8)
    a, m = serve._device_inputs(img, Image.fromarray(sk))
    assert a.dtype == np.uint8 and a.shape == (67, 70, 3) and np.array_equal(m, sk)
    sk3 = rng.randint(0, 256, (50, 41, 3)).astype(np.uint8)
    _, m3 = serve._device_inputs(img, Image.fromarray(sk3))
    assert np.array_equal(m3, sk3[..., 0]) and m3.flags.c_contiguous
    host = np.array(Image.fromarray(sk3).resize((64, 64)))[..., 0]
    assert np.array_equal(R.resize(m3, (64, 64)), host)
    for mode in ("1", "P", "RGBA"):
        assert serve._device_inputs(img, Image.new(mode, (41, 50))) is None
    with pytest.raises(ValueError):
        serve._device_inputs(Image.new("RGB", (12, 40)), Image.new("L", (12, 40)))
