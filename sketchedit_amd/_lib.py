"""ctypes binding of libsketchedit_hip.so (C-ABI in include/sketchedit_hip.h).

This is the thin layer a maintainer of the reference would add: torch owns the
device tensors, this module passes their raw pointers + the current HIP stream to the library.
There is NO fallback: if the library is missing or fails, an exception is raised.
"""
import contextlib
import ctypes
import os
import subprocess
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SKETCHEDIT_HIP_LIB points at another build of the same library (developer builds, e.g. tools/wino_trace.py)
LIB_PATH = os.environ.get("SKETCHEDIT_HIP_LIB") or os.path.join(_HERE, "lib", "libsketchedit_hip.so")
CSRC = os.path.join(_HERE, "csrc")
SOURCES = ["se_gconv.hip", "se_rconv16.hip", "se_rconv96.hip", "se_rtile.hip", "se_rtilew.hip", "se_wino.hip", "se_wino24.hip", "se_wino48.hip", "se_wino_up.hip", "se_wino_up48.hip", "se_s2poly.hip", "se_attention.hip", "se_att_stream.hip", "se_misc.hip", "se_resize.hip",
           "se_window.hip", "se_feather.hip", "se_fill.hip", "se_select.hip", "se_lasso.hip", "se_modify.hip", "se_outline.hip", "se_move.hip", "se_blend.hip", "se_canvas.hip", "se_warp.hip", "se_filter.hip", "se_adjust.hip", "se_png.hip", "se_jpg.hip", "se_pack.hip",
           "se_plan.hip", "se_api_window.hip", "se_api_select.hip", "se_api_move.hip", "se_api_codec.hip", "se_api_debug.hip", "se_api.hip"]

SE_NET_G, SE_NET_M = 0, 1
RESAMPLE_LANCZOS, RESAMPLE_BILINEAR, RESAMPLE_BICUBIC = 1, 2, 3   # se_resize_u8 filters = PIL.Image.Resampling values
FLAG_USE_CAM, FLAG_POOL_MAX, FLAG_NO_MASK_CC, FLAG_NO_MASK_COARSE, FLAG_JOINT_TRAIN_INP = 1, 2, 4, 8, 16
FLAG_LOW_LATENCY, FLAG_GRAPH, FLAG_PACKED_OUT, FLAG_BF16, FLAG_CONSERVATIVE = 32, 64, 128, 256, 512   # execution options (include/sketchedit_hip.h)
FLAG_RAW_FINE = 1024   # se_fill_window_u8 only: rgb is the quantised `fine`, uncomposed
# Which calls run in the low-latency mode unless the caller says otherwise: at most three 256x256 images' worth of pixels, or ONE
# image of up to 512x512.  Re-measured on MI355X in round 6 (tools/ll_threshold.sh), low-latency vs default, after the default
# mode learned to overlap netG's branches and the low-latency mode to keep the Winograd kernels where ONE image's grid still
# covers the chip: 256x256 B = 1 / 2 / 3 / 4: 1.20 / 1.75 / 2.45 / 3.05 ms vs 2.33 / 2.43 / 2.54 / 2.66; 384x384 B = 1: 2.02 vs
# 2.59; 512x512 B = 1 / 2: 2.84 / 3.86 vs 2.96 / 3.80
LOW_LATENCY_MAX_PIXELS = 3 * 256 * 256
LOW_LATENCY_MAX_SINGLE_IMAGE = 512 * 512

# The #define'd limits and codes of include/*.h, each once on the Python side: SE_<NAME> is <NAME> here (tests/test_abi_host.py
# holds every define against its mirror).  serve.py imports them from here
SE_JPG_420, SE_JPG_OPTIMIZE = 1, 2            # the flags of sketchedit_jpg2.h
JPG_TABLE_RECORD_BYTES = 1088                 # one image's four tables as se_jpg2_encode_u8 leaves them
FEATHER_MAX_RADIUS = 16
SELECT_MAX_GROW, SELECT_MAX_PASSES = 16, 64
LASSO_MAX_EDGES, LASSO_MAX_EXTENT = 65536, 8192
COMBINE_ADD, COMBINE_SUBTRACT, COMBINE_INTERSECT, COMBINE_XOR, COMBINE_INVERT = range(5)
OUTLINE_TILE, OUTLINE_MAX_CAP = 64, 1 << 24
MOVE_MAX_OFFSET, MOVE_MAX_RADIUS = 16384, 16
MOVE_FLIP_X, MOVE_FLIP_Y = 1, 2
BLEND_MAX_SIDE = 2048
CANVAS_MIRROR_X, CANVAS_MIRROR_Y, CANVAS_TRANSPOSE = 1, 2, 4
CANVAS_EDGE, CANVAS_REFLECT, CANVAS_CONSTANT = 0, 1, 2
CANVAS_MAX_SIDE, CANVAS_MAX_OFFSET = 32768, 1 << 20
WARP_MAX_COEF, WARP_MAX_TRANSLATION = 1 << 20, 1 << 40
FILTER_MAX_RADIUS, FILTER_ONE, FILTER_MAX_CELL = 32, 4096, 64
FILTER_MIN_AMOUNT, FILTER_MAX_AMOUNT, FILTER_MAX_FEATHER = -256, 1024, 16
ADJUST_MAX_COEF, ADJUST_MAX_OFFSET, ADJUST_ONE_AMOUNT = 32768, 1 << 20, 256
ADJUST_MAX_FEATHER, ADJUST_MAX_CLIP, ADJUST_HIST_GROUPS = 16, 200, 256
ADJUST_STRETCH, ADJUST_EQUALIZE, ADJUST_MATCH = 0, 1, 2
ADJUST_PER_CHANNEL, ADJUST_LUMA = 0, 1
MODIFY_MAX_RADIUS = 32
MODIFY_EXPAND, MODIFY_CONTRACT, MODIFY_SMOOTH = range(3)


class SketchEditHipError(RuntimeError):
    pass


class NetGTaps(ctypes.Structure):
    """se_netG_taps (include/sketchedit_hip.h): optional intermediate outputs of netG, device pointers or NULL"""
    _fields_ = [("pmconv6", ctypes.c_void_p), ("attn_out", ctypes.c_void_p), ("style_vec", ctypes.c_void_p)]


class Window(ctypes.Structure):
    """se_window (include/sketchedit_hip.h): one request of a window edit -- its resident frame, the window's sketch (device
    pointers) and where the window lies in the frame"""
    _fields_ = [("frame_u8", ctypes.c_void_p), ("sketch_u8", ctypes.c_void_p), ("Hi", ctypes.c_int), ("Wi", ctypes.c_int),
                ("y0", ctypes.c_int), ("x0", ctypes.c_int)]


class OutputConvIO(ctypes.Structure):
    """se_output_conv_io (include/sketchedit_hip.h): the optional tensors of the output conv's epilogue, device pointers or NULL"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("out", "hard", "lock", "img", "mask", "xnow", "composed", "rgb8", "m8")]


# The C ABI, one row per entry: (name, restype, argtypes), keyed by the header that declares it, in the header's order.
# load_library() binds every row; tests/test_abi_host.py holds the rows against the prototypes and the library's exports
vp, ci, cu, sz, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_char_p      # vp: device and host addresses alike
pvp, pci, pw = ctypes.POINTER(vp), ctypes.POINTER(ci), ctypes.POINTER(Window)
ABI = {
    "sketchedit_hip.h": [
        ("se_create", ci, [ci, pvp]),
        ("se_destroy", None, [vp]),
        ("se_last_error", cs, [vp]),
        ("se_version", cs, []),
        ("se_load_weights", ci, [vp, ci, cs, vp, pci, ci]),
        ("se_weights_ready", ci, [vp]),
        ("se_workspace_bytes", sz, [vp, ci, ci, ci]),
        ("se_netM_forward", ci, [vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci]),
        ("se_netM_forward_ex", ci, [vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci]),
        ("se_netG_forward", ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci]),
        ("se_netG_forward_taps", ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci, ctypes.POINTER(NetGTaps)]),
        ("se_inference", ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci]),
        ("se_inference_u8", ci, [vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci]),
        ("se_dequantize_u8", ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci]),
        ("se_inference_u8io", ci, [vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci]),
        ("se_quantize_u8", ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci]),
        ("se_resize_u8", ci, [vp, vp, vp, ci, ci, ci, ci, vp, ci, ci, ci]),
        ("se_prepare_u8", ci, [vp, vp, vp, ci, ci, vp, ci, ci, vp, vp, ci, ci]),
        ("se_edit_u8", ci, [vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci, ci, ci]),
        ("se_edit_u8_workspace_bytes", sz, [vp, ci, ci, ci]),
        ("se_window_gather_u8", ci, [vp, vp, pw, ci, ci, ci, vp, vp]),
        ("se_window_border_u8", ci, [vp, vp, pw, ci, ci, ci, vp, vp]),
        ("se_window_paste_u8", ci, [vp, vp, pw, ci, ci, ci, vp, vp]),
        ("se_edit_window_u8", ci, [vp, vp, pw, ci, ci, ci, vp, vp, vp, ci, vp, sz, ci]),
        ("se_edit_window_u8_workspace_bytes", sz, [vp, ci, ci, ci]),
        ("se_window_gather_resize_u8", ci, [vp, vp, pw, ci, ci, ci, ci, ci, vp, vp]),
        ("se_window_paste_resize_u8", ci, [vp, vp, pw, ci, ci, ci, ci, ci, vp, vp]),
        ("se_edit_window_scaled_u8", ci, [vp, vp, pw, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, sz, ci]),
        ("se_edit_window_scaled_u8_workspace_bytes", sz, [vp, ci, ci, ci, ci, ci]),
        ("se_window_saved_bytes", sz, [ci, ci]),
        ("se_window_save_u8", ci, [vp, vp, pw, ci, ci, ci, pvp]),
        ("se_window_swap_u8", ci, [vp, vp, pw, ci, ci, ci, pvp]),
        ("se_inference_locked", ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci]),
        ("se_inference_u8_locked", ci, [vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci]),
        ("se_window_gather_lock_u8", ci, [vp, vp, pw, pvp, ci, ci, ci, ci, ci, vp]),
        ("se_window_paste_locked_u8", ci, [vp, vp, pw, pvp, ci, ci, ci, ci, ci, vp, vp]),
        ("se_edit_window_locked_u8", ci, [vp, vp, pw, pvp, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, sz, ci]),
        ("se_edit_window_locked_u8_workspace_bytes", sz, [vp, ci, ci, ci, ci, ci]),
        ("se_sketch_tiles_u8", ci, [vp, vp, vp, ci, ci, ci, vp]),
        ("se_sketch_strokes_u8", ci, [vp, vp, vp, ci, ci, ci, vp, ci, vp, vp]),
        ("se_resample_coeffs", ci, [ci, ci, ci, vp, vp, sz]),
        ("se_profile_enable", ci, [vp, ci]),
        ("se_profile_report", ci, [vp, cs, sz]),
        ("se_debug_set_option", ci, [cs, ci]),
        ("se_debug_get_option", ci, [cs, pci]),
        ("se_debug_reset_options", None, []),
        ("se_debug_gconv_form", ci, [ci] * 14 + [cs, sz]),
        ("se_gated_conv2d", ci, [vp, vp, vp, vp, vp, vp] + [ci] * 10),
        ("se_gated_conv2d_ex", ci, [vp, vp, vp, vp, ci, vp, vp, vp] + [ci] * 12),
        ("se_attention", ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci]),
        ("se_attention_ex", ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci]),
        ("se_pack_inputs", ci, [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci]),
        ("se_column_reduce", ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci]),
        ("se_output_conv", ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(OutputConvIO), ci, ci, ci]),
    ],
    "sketchedit_png.h": [
        ("se_png_bound", sz, [ci, ci]),
        ("se_png_encode_u8", ci, [vp, vp, pw, ci, ci, ci, vp, sz, vp, vp, sz]),
        ("se_png_encode_u8_workspace_bytes", sz, [vp, ci, ci, ci]),
    ],
    "sketchedit_jpg.h": [
        ("se_jpg_bound", sz, [ci, ci]),
        ("se_jpg_encode_u8", ci, [vp, vp, pw, ci, ci, ci, ci, vp, sz, vp, vp, sz]),
        ("se_jpg_encode_u8_workspace_bytes", sz, [vp, ci, ci, ci]),
    ],
    "sketchedit_jpg2.h": [
        ("se_jpg2_bound", sz, [ci, ci, ci]),
        ("se_jpg2_encode_u8", ci, [vp, vp, pw, ci, ci, ci, ci, ci, vp, sz, vp, vp, vp, sz]),
        ("se_jpg2_encode_u8_workspace_bytes", sz, [vp, ci, ci, ci, ci]),
        ("se_jpg2_code_i16", ci, [vp, vp, vp, ci, ci, ci, ci, vp, sz, vp, vp, vp, sz]),
        ("se_jpg2_code_i16_workspace_bytes", sz, [vp, ci, ci, ci, ci]),
    ],
    "sketchedit_feather.h": [
        ("se_window_paste_feather_u8", ci, [vp, vp, pw, pvp, ci, ci, ci, ci, vp, vp]),
    ],
    "sketchedit_fill.h": [
        ("se_fill", ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci]),
        ("se_fill_window_u8_workspace_bytes", sz, [vp, ci, ci, ci, ci, ci]),
        ("se_fill_window_u8", ci, [vp, vp, pw, pvp, pvp, ci, ci, ci, ci, ci, vp, vp, vp, sz, ci]),
        ("se_fill_keep_u8", ci, [vp, vp, pw, pvp, pvp, pvp, ci, ci, ci]),
    ],
    "sketchedit_select.h": [
        ("se_select_similar_u8", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
        ("se_select_flood_u8", ci, [vp, vp, vp, ci, ci, ci, vp]),
        ("se_select_grow_u8", ci, [vp, vp, vp, ci, ci, ci, vp]),
    ],
    "sketchedit_lasso.h": [
        ("se_lasso_fill_u8", ci, [vp, vp, vp, ci, ci, ci, vp]),
        ("se_plane_combine_u8", ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    ],
    "sketchedit_outline.h": [
        ("se_outline_u8_workspace_bytes", sz, [vp, ci, ci]),
        ("se_outline_u8", ci, [vp, vp, vp, ci, ci, vp, ci, vp, vp, sz]),
    ],
    "sketchedit_move.h": [
        ("se_move_drop_u8", ci, [vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, vp, vp] + [ci] * 8),
        ("se_plane_shift_u8", ci, [vp, vp, vp, ci, ci] + [ci] * 7 + [vp]),
    ],
    "sketchedit_warp.h": [
        ("se_warp_drop_u8", ci, [vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, vp, vp] + [ci] * 8 + [vp]),
        ("se_plane_warp_u8", ci, [vp, vp, vp, ci, ci] + [ci] * 4 + [vp, vp]),
    ],
    "sketchedit_filter.h": [
        ("se_filter_blur_u8", ci, [vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, vp, vp] + [ci] * 4 + [vp, ci, ci, ci]),
        ("se_filter_mosaic_u8", ci, [vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, vp, vp] + [ci] * 7),
    ],
    "sketchedit_adjust.h": [
        ("se_adjust_u8", ci, [vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, vp, vp] + [ci] * 4 + [vp, vp, ci, ci]),
        ("se_adjust_hist_u8_workspace_bytes", sz, [ci, ci]),
        ("se_adjust_hist_u8", ci, [vp, vp, vp, ci, ci, vp] + [ci] * 4 + [vp, vp, sz]),
        ("se_adjust_lut_u8", ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    ],
    "sketchedit_modify.h": [
        ("se_plane_modify_u8", ci, [vp, vp, vp, ci, ci, ci, ci, vp]),
    ],
    "sketchedit_blend.h": [
        ("se_move_blend_u8_workspace_bytes", sz, [ci, ci]),
        ("se_move_blend_u8", ci, [vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, vp, vp] + [ci] * 7 + [vp, sz]),
    ],
    "sketchedit_canvas.h": [
        ("se_canvas_u8", ci, [vp, vp, vp, ci, ci, ci, vp, ci, ci, ci, ci, ci, ci, cu]),
    ],
}
# bound when present: a build from before the entry still loads through SKETCHEDIT_HIP_LIB
ABI_OPTIONAL = {"se_debug_gconv_form"}


def abi_names(header=None):
    """The entry names one header declares ("sketchedit_png.h"), in its order, or with no header those of all"""
    return [row[0] for h in ([header] if header else ABI) for row in ABI[h]]


def build_library(force=False, verbose=False, extra_flags=()):
    """hipcc --offload-arch=gfx950 -> sketchedit_amd/lib/libsketchedit_hip.so (cross-compiles without a GPU).
    One object per source, compiled in parallel; an object is rebuilt when its source or a header is newer OR when its
    command line changed (flags / -D macros: the command is kept beside the object), then one link.  The whole build holds
    an exclusive file lock, so concurrent builders (ranks, test workers) do not write the same objects."""
    import fcntl
    from concurrent.futures import ThreadPoolExecutor
    import glob
    hdrs = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(_HERE, "..", "include", "*.h"))
    hdr_t = max(os.path.getmtime(h) for h in hdrs)
    objdir = os.path.join(_HERE, "lib", "obj")
    os.makedirs(objdir, exist_ok=True)
    with open(os.path.join(_HERE, "lib", ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        jobs, objs = [], []
        for src in SOURCES:
            sp, op = os.path.join(CSRC, src), os.path.join(objdir, src.replace(".hip", ".o"))
            objs.append(op)
            cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + list(extra_flags) + ["-c", sp, "-o", op]
            try:
                with open(op + ".cmd") as f:
                    same_cmd = f.read() == " ".join(cmd)
            except OSError:
                same_cmd = False
            if force or not same_cmd or not os.path.exists(op) or os.path.getmtime(op) < max(os.path.getmtime(sp), hdr_t):
                jobs.append(cmd)
        if not jobs and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(o) for o in objs):
            return LIB_PATH

        def run(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            if "-c" in cmd:
                with open(cmd[-1] + ".cmd", "w") as f:
                    f.write(" ".join(cmd))
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1) or 1) as ex:
            list(ex.map(run, jobs))
        run(["hipcc", "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIB_PATH + ".tmp"] + objs)
        os.replace(LIB_PATH + ".tmp", LIB_PATH)          # readers never see a half-written library
    return LIB_PATH


_lib = None
_lib_lock = threading.Lock()


def load_library():
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise SketchEditHipError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU or PyTorch fallback for this path)" % LIB_PATH)
        # PyTorch first: it brings its own HIP runtime (torch/lib/libamdhip64.so) and our library must bind to that one.
        # Loaded the other way round the process ends up with two HIP runtimes and hipGetDeviceCount() returns 0.
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for rows in ABI.values():
            for name, restype, argtypes in rows:
                if name in ABI_OPTIONAL and not hasattr(lib, name):
                    continue
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return lib


_shared = {}
_shared_lock = threading.Lock()


def shared_engine(device=0):
    """A process-wide Engine per device for the per-op entry points (no weights involved)."""
    with _shared_lock:
        if device not in _shared:
            _shared[device] = Engine(device)
        return _shared[device]


def set_option(name, value):
    """Developer switch of the library, process-wide, effective from the next call on.  The library
    reads its switches from the environment ONCE; tests and A/B tools change them afterwards through this call."""
    if load_library().se_debug_set_option(name.encode(), int(value)):
        raise SketchEditHipError("unknown developer switch %r" % name)


def get_option(name):
    v = ctypes.c_int(0)
    if load_library().se_debug_get_option(name.encode(), ctypes.byref(v)):
        raise SketchEditHipError("unknown developer switch %r" % name)
    return v.value


def reset_options():
    load_library().se_debug_reset_options()


def gconv_form(cin, cout, H, W, k=3, stride=1, rate=1, act="elu", upsample=False, cin1=0, x1_is_vector=False, B=1,
               low_latency=False, bf16=False, conservative=False, net=SE_NET_G):
    """The conv launches gated_conv2d would make for this call, as a list of form names (['vecbias', 'wino24'], ['small_conv']):
    se_debug_gconv_form, the library's own rule (choose_form) evaluated on the host -- no device, nothing runs.  cin: the first
    source's channels; cin1: the second's (0: none)."""
    flags = (FLAG_LOW_LATENCY if low_latency else 0) | (FLAG_BF16 if bf16 else 0) | (FLAG_CONSERVATIVE if conservative else 0)
    buf = ctypes.create_string_buffer(64)
    if load_library().se_debug_gconv_form(cin, cin1, int(bool(x1_is_vector)), cout, k, stride, rate,
                                          {"elu": 0, "relu": 1, None: 2}[act], int(bool(upsample)), B, H, W, flags, net, buf, len(buf)):
        raise SketchEditHipError("gconv_form: not a layer gated_conv2d takes")
    return buf.value.decode().split(",")


def s2poly_tables():
    """The 1-D tables of the polyphase F(2,2) form (csrc/se_s2poly.h) as a (5, 7) int32 array: per position [source +, source -
    (or -1), coefficient of w0, w1, w2, fold into o0, o1] -- the derived entry "SE_S2POLY_TABLE:q,j" of se_debug_get_option, no
    device."""
    return np.array([[get_option("SE_S2POLY_TABLE:%d,%d" % (q, j)) for j in range(7)] for q in range(5)], np.int32)


def s2poly_probe_layer(cout):
    """The probe layer of include/sketchedit_hip.h ("SE_S2POLY_PACK"): w (cout,48,3,3) and b (cout,) float32, every value a
    multiple of 1/1024 below 1.01 in magnitude."""
    p = lambda n: (((7919 * n) % 2053 - 1026) / 1024.0).astype(np.float32)      # noqa: E731
    return p(np.arange(cout * 48 * 9, dtype=np.int64)).reshape(cout, 48, 3, 3), p(10007 + np.arange(cout, dtype=np.int64))


def s2poly_probe_pack(cout):
    """The weight image (cout/96, 38, 96, 32) and bias (cout,) the library's packer builds for s2poly_probe_layer(cout), cout 96 or
    192, read float by float through the derived entry "SE_S2POLY_PACK:cout,i" of se_debug_get_option -- host only, no device."""
    fn = load_library().se_debug_get_option
    n = (cout // 96) * 38 * 96 * 32
    out = np.zeros(n + cout, np.int32)
    v = ctypes.c_int(0)
    for i in range(n + cout):
        if fn(("SE_S2POLY_PACK:%d,%d" % (cout, i)).encode(), ctypes.byref(v)):
            raise SketchEditHipError("SE_S2POLY_PACK: cout must be 96 or 192")
        out[i] = v.value
    f = out.view(np.float32)
    return f[:n].reshape(cout // 96, 38, 96, 32).copy(), f[n:].copy()


def pair_rule(B, H, W, low_latency=False):
    """Whether the forwards run a pass of B images of H x W as two half-batch chains on two streams: the library's own rule
    (se_host.h pair_rule, SE_PAIR_MIN_PIXELS included) asked on the host through the derived entry "SE_PAIR_RULE:B,H,W,flags" of
    se_debug_get_option -- no device, nothing runs.  Results never depend on the answer."""
    v = ctypes.c_int(-1)
    name = "SE_PAIR_RULE:%d,%d,%d,%d" % (B, H, W, FLAG_LOW_LATENCY if low_latency else 0)
    if load_library().se_debug_get_option(name.encode(), ctypes.byref(v)):
        raise SketchEditHipError("pair_rule: bad shape B=%d H=%d W=%d" % (B, H, W))
    return bool(v.value)


def flags_from_opt(opt):
    """netG flag word from a reference-style options namespace (editline_g.py:15-23, base_options.py:19)."""
    f = 0
    if getattr(opt, "use_cam", False):
        f |= FLAG_USE_CAM
    pool = getattr(opt, "pool_type", "avg")
    if pool == "max":
        f |= FLAG_POOL_MAX
    elif pool != "avg":
        raise NotImplementedError(pool)        # editline_g.py:164-165
    if getattr(opt, "no_mask_cc", False):
        f |= FLAG_NO_MASK_CC
    if getattr(opt, "no_mask_coarse", False):
        f |= FLAG_NO_MASK_COARSE
    if getattr(opt, "joint_train_inp", False):
        f |= FLAG_JOINT_TRAIN_INP
    return f


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check_dev(*ts):
    import torch
    for t in ts:
        if t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise SketchEditHipError("expected contiguous float32 CUDA(HIP) tensors")


def upload_u8(a, device):
    """A uint8 array (numpy or tensor) on the device.  np.asarray of a PIL image is read-only: torch warns about wrapping it
    without a copy, but the wrapper is only read, to upload it."""
    import warnings
    import torch
    if isinstance(a, np.ndarray):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device, non_blocking=True).contiguous()


def _check_dev_u8(*ts):
    import torch
    for t in ts:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise SketchEditHipError("expected contiguous uint8 CUDA(HIP) tensors")


class Engine:
    """One se_ctx on one GPU + its workspace.  Thread-safe (the library serialises forwards per ctx)."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise SketchEditHipError("no HIP device visible: the sketchedit_amd forward only runs on an MI355X")
        self.lib = load_library()
        self.device = int(device)
        h = ctypes.c_void_p()
        if self.lib.se_create(self.device, ctypes.byref(h)) != 0:
            raise SketchEditHipError("se_create: " + self.lib.se_last_error(None).decode())
        self.h = h
        self._ws = None
        self._ws_lock = threading.Lock()
        self._ws_stream = None
        self._graph_stream = None
        self.precision = "f32"     # "bf16": BASELINE config 5 (bf16 storage + MFMA, fp32 accumulate); see set_precision
        self.conservative = False  # SE_FLAG_CONSERVATIVE on every forward: netM's 96 -> 192 layers on F(2x2,3x3) (set_conservative)
        self._static = {}          # graph mode: per-shape input copies and output buffers (stable pointers)
        self._graph_lock = threading.Lock()    # graph mode is single-caller per Engine: one replay at a time

    def close(self):
        if getattr(self, "h", None):
            self.lib.se_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what):
        raise SketchEditHipError("%s: %s" % (what, self.lib.se_last_error(self.h).decode()))

    # ---- weights -------------------------------------------------------------------------------
    def load_state_dict(self, net, state_dict):
        """net in {'G','M'}; state_dict: key -> array/tensor in checkpoint layout (strict)."""
        net_id = SE_NET_G if net == "G" else SE_NET_M
        for k, v in state_dict.items():
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (ctypes.c_int * a.ndim)(*a.shape)
            if self.lib.se_load_weights(self.h, net_id, k.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim):
                self._err("se_load_weights(%s)" % k)

    def weights_ready(self):
        return bool(self.lib.se_weights_ready(self.h))

    # ---- workspace -----------------------------------------------------------------------------
    def workspace(self, B, H, W):
        need = self.lib.se_workspace_bytes(self.h, B, H, W)
        if need == 0:
            self._err("se_workspace_bytes")
        return self._workspace_bytes(need)

    def _workspace_bytes(self, need):
        import torch
        with self._ws_lock:
            cur = torch.cuda.current_stream(self.device)
            if self._ws is None or self._ws.numel() < need:
                if self._ws is not None:
                    # earlier forwards may still be using the old block on their stream: keep the caching allocator
                    # from handing it out before they finish
                    self._ws.record_stream(self._ws_stream)
                self._ws = torch.empty(need, dtype=torch.uint8, device="cuda:%d" % self.device)
                with self._graph_lock:     # (never taken in the other order: the graph path asks for the workspace first)
                    self._static.clear()   # captured graphs are keyed by the workspace pointer
            elif self._ws_stream is not None and self._ws_stream != cur:
                # one workspace = one stream: forwards on another stream must not overlap the previous ones
                cur.wait_stream(self._ws_stream)
            self._ws_stream = cur
            return self._ws

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- forwards ------------------------------------------------------------------------------
    def netM(self, image, sketch, want_image=True):
        import torch
        _check_dev(image, sketch)
        B, _, H, W = image.shape
        ws = self.workspace(B, H, W)
        mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=image.device)
        mim = torch.empty((B, 3, H, W), dtype=torch.float32, device=image.device) if want_image else None
        if self.lib.se_netM_forward_ex(self.h, self._stream(), _ptr(image), _ptr(sketch), _ptr(mask), _ptr(mim),
                                       _ptr(ws), ws.numel(), B, H, W,
                                       (FLAG_BF16 if self.precision == "bf16" else 0) | (FLAG_CONSERVATIVE if self.conservative else 0)):
            self._err("se_netM_forward_ex")
        return mask, mim

    def netG(self, x, x2, mask, mask2, guide, flags):
        import torch
        _check_dev(x, x2, mask, mask2, guide)
        B, _, H, W = x.shape
        ws = self.workspace(B, H, W)
        coarse = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
        fine = torch.empty_like(coarse)
        flags = (flags & 31) | (FLAG_BF16 if self.precision == "bf16" else 0)
        if self.lib.se_netG_forward(self.h, self._stream(), _ptr(x), _ptr(x2), _ptr(mask), _ptr(mask2), _ptr(guide),
                                    _ptr(coarse), _ptr(fine), _ptr(ws), ws.numel(), B, H, W, flags):
            self._err("se_netG_forward")
        return coarse, fine

    def netG_taps(self, x, x2, mask, mask2, guide, flags):
        """netG with its intermediate outputs (se_netG_forward_taps; the counterparts of the forward hooks
        tests/golden/make_golden.py puts on the reference): -> dict(coarse, fine, pmconv6, attn_out, style_vec).  The
        attention runs in the form the production forward uses."""
        import torch
        _check_dev(x, x2, mask, mask2, guide)
        B, _, H, W = x.shape
        ws = self.workspace(B, H, W)
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)     # noqa: E731
        r = dict(coarse=mk(B, 3, H, W), fine=mk(B, 3, H, W), pmconv6=mk(B, 96, H // 4, W // 4), style_vec=mk(B, 96))
        if flags & FLAG_USE_CAM:
            r["attn_out"] = mk(B, 96, H // 4, W // 4)
        taps = NetGTaps(r["pmconv6"].data_ptr(), r["attn_out"].data_ptr() if "attn_out" in r else None, r["style_vec"].data_ptr())
        flags = (flags & 31) | (FLAG_BF16 if self.precision == "bf16" else 0)
        if self.lib.se_netG_forward_taps(self.h, self._stream(), _ptr(x), _ptr(x2), _ptr(mask), _ptr(mask2), _ptr(guide),
                                         _ptr(r["coarse"]), _ptr(r["fine"]), _ptr(ws), ws.numel(), B, H, W, flags, ctypes.byref(taps)):
            self._err("se_netG_forward_taps")
        return r

    def set_conservative(self, on=True):
        """SE_FLAG_CONSERVATIVE (include/sketchedit_hip.h): netM -- whose soft mask feeds the hard 0.5 threshold -- keeps the
        F(2x2,3x3) Winograd form; netG keeps the hybrid one.  +1.7 % per step at 256x256 batch 32."""
        self.conservative = bool(on)

    def set_precision(self, precision):
        """'f32' (default; the north star's 1e-3 parity bound applies) or 'bf16' (SE_FLAG_BF16 on every forward)."""
        if precision not in ("f32", "bf16"):
            raise ValueError(precision)
        self.precision = precision

    @staticmethod
    def is_low_latency(B, H, W, low_latency=None):
        """The low-latency mode is chosen by call size unless forced (True / False)."""
        if low_latency is not None:
            return bool(low_latency)
        return B * H * W <= LOW_LATENCY_MAX_PIXELS or (B == 1 and H * W <= LOW_LATENCY_MAX_SINGLE_IMAGE)

    def exec_flags(self, B, H, W, low_latency=None, graph=False):
        """Execution-option bits for a call."""
        return (FLAG_LOW_LATENCY if self.is_low_latency(B, H, W, low_latency) else 0) | (FLAG_GRAPH if graph else 0) | \
            (FLAG_BF16 if self.precision == "bf16" else 0) | (FLAG_CONSERVATIVE if self.conservative else 0)

    def inference(self, image, sketch, flags, visualize=False, out=None, low_latency=None, graph=False, lock=None):
        """-> dict(composed, mask[, hard, maskim, coarse, fine]).  `out` may hold preallocated composed/mask.

        lock: a (B,H,W) uint8 tensor on the device, non-zero = locked -- the soft mask is 0 there before the
        threshold, so netG sees those pixels as known context and composed keeps the image's bits (se_inference_locked;
        graph=True is ignored with a lock).

        low_latency: None = by size (small calls), True / False = forced.  graph=True replays the forward from a
        captured hipGraph: that needs stable pointers, so the inputs are copied into buffers this Engine keeps per
        shape and the returned tensors ARE the per-shape output buffers -- consume them before the next call of the
        same shape."""
        import torch
        _check_dev(image, sketch)
        if lock is not None:
            self._check_lock(lock, image)
            graph = False
        if graph and out is not None:
            raise SketchEditHipError("graph=True replays into buffers the Engine keeps per shape: `out=` cannot be honoured "
                                     "(copy from the returned tensors, or call without graph=True)")
        B, _, H, W = image.shape
        ws = self.workspace(B, H, W)
        dev = image.device
        flags = (flags & 31) | self.exec_flags(B, H, W, low_latency, graph)

        def new_outputs(have=None):
            mk = lambda c: torch.empty((B, c, H, W), dtype=torch.float32, device=dev)     # noqa: E731
            o = dict(composed=have["composed"], mask=have["mask"]) if have else dict(composed=mk(3), mask=mk(1))
            if visualize:
                o.update(hard=mk(1), maskim=mk(3), coarse=mk(3), fine=mk(3))
            return o

        if graph:
            # the per-shape input copies, the launch and the (shared) output buffers form one critical section: two threads
            # replaying the same shape would otherwise overwrite each other's inputs / read each other's outputs.  The
            # returned tensors ARE the static buffers, so a second graph call of the same shape must wait until the first
            # caller has consumed them: graph mode is documented single-caller, the lock only keeps a concurrent call from
            # corrupting a replay in flight.
            with self._graph_lock:
                return self._inference_graph(image, sketch, flags, visualize, ws, B, H, W, new_outputs)
        r = new_outputs(out)
        self._call_inference(image, sketch, r, ws, B, H, W, flags, self._stream(), lock)
        return r

    @staticmethod
    def _check_lock(lock, image):
        _check_dev_u8(lock)
        B, _, H, W = image.shape
        if tuple(lock.shape) != (B, H, W):
            raise SketchEditHipError("lock: expected a (B,H,W) uint8 plane of the images' size")

    def _call_inference(self, image, sketch, r, ws, B, H, W, flags, stream, lock=None):
        if lock is not None:
            if self.lib.se_inference_locked(self.h, stream, _ptr(image), _ptr(sketch), _ptr(lock), _ptr(r["composed"]),
                                            _ptr(r["mask"]), _ptr(r.get("hard")), _ptr(r.get("maskim")), _ptr(r.get("coarse")),
                                            _ptr(r.get("fine")), _ptr(ws), ws.numel(), B, H, W, flags):
                self._err("se_inference_locked")
            return
        if self.lib.se_inference(self.h, stream, _ptr(image), _ptr(sketch), _ptr(r["composed"]), _ptr(r["mask"]),
                                 _ptr(r.get("hard")), _ptr(r.get("maskim")), _ptr(r.get("coarse")), _ptr(r.get("fine")),
                                 _ptr(ws), ws.numel(), B, H, W, flags):
            self._err("se_inference")

    def _inference_graph(self, image, sketch, flags, visualize, ws, B, H, W, new_outputs):
        import torch
        key = (B, H, W, bool(visualize))
        st = self._static.get(key)
        if st is None:
            st = self._static[key] = {"image": torch.empty_like(image), "sketch": torch.empty_like(sketch),
                                      "outs": new_outputs()}
        st["image"].copy_(image)
        st["sketch"].copy_(sketch)
        image, sketch = st["image"], st["sketch"]
        r = dict(st["outs"])
        # stream capture is not permitted on the legacy default stream: graph-mode forwards run on a stream of their
        # own, ordered after / before the caller's current stream
        cur = torch.cuda.current_stream(self.device)
        if self._graph_stream is None:
            self._graph_stream = torch.cuda.Stream(device=self.device)
        gs = self._graph_stream
        gs.wait_stream(cur)
        self._call_inference(image, sketch, r, ws, B, H, W, flags, ctypes.c_void_p(gs.cuda_stream))
        cur.wait_stream(gs)
        return r

    def inference_u8(self, image, sketch, flags, low_latency=None, lock=None):
        """The forward with test.py:25-27's quantisation fused into its last kernel -> (rgb (B,H,W,3) uint8, mask (B,H,W)
        uint8): what test.py writes to disk, without an fp32 output tensor or a separate pass.  lock: as `inference`."""
        import torch
        _check_dev(image, sketch)
        if lock is not None:
            self._check_lock(lock, image)
        B, _, H, W = image.shape
        ws = self.workspace(B, H, W)
        rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=image.device)
        m8 = torch.empty((B, H, W), dtype=torch.uint8, device=image.device)
        flags = (flags & 31) | self.exec_flags(B, H, W, low_latency, False)
        if lock is not None:
            if self.lib.se_inference_u8_locked(self.h, self._stream(), _ptr(image), _ptr(sketch), _ptr(lock), _ptr(rgb), _ptr(m8),
                                               _ptr(ws), ws.numel(), B, H, W, flags):
                self._err("se_inference_u8_locked")
        elif self.lib.se_inference_u8(self.h, self._stream(), _ptr(image), _ptr(sketch), _ptr(rgb), _ptr(m8), _ptr(ws),
                                      ws.numel(), B, H, W, flags):
            self._err("se_inference_u8")
        return rgb, m8

    def dequantize_u8(self, image_u8, sketch_u8):
        """data/testimage_dataset.py:89-111 on the device: (B,H,W,3) uint8 RGB, (B,H,W) uint8 'L' -> image (B,3,H,W) fp32 in
        [-1,1] = (v/255 - 0.5)/0.5, sketch (B,1,H,W) fp32 in {0,1} = (v > 0); bit-identical to the CPU dataset's tensors."""
        import torch
        _check_dev_u8(image_u8, sketch_u8)
        B, H, W, _ = image_u8.shape
        image = torch.empty((B, 3, H, W), dtype=torch.float32, device=image_u8.device)
        sketch = torch.empty((B, 1, H, W), dtype=torch.float32, device=image_u8.device)
        if self.lib.se_dequantize_u8(self.h, self._stream(), _ptr(image_u8), _ptr(sketch_u8), _ptr(image), _ptr(sketch), B, H, W):
            self._err("se_dequantize_u8")
        return image, sketch

    def inference_u8io(self, image_u8, sketch_u8, flags, low_latency=None, out=None):
        """uint8 in, uint8 out: test.py:20-37 between the PNG decoder and the PNG encoder as ONE library call
        (se_inference_u8io).  image_u8 (B,H,W,3), sketch_u8 (B,H,W) -> (rgb (B,H,W,3), mask (B,H,W)), all uint8 on the device.
        `out` = (rgb, mask) preallocated."""
        import torch
        _check_dev_u8(image_u8, sketch_u8)
        B, H, W, _ = image_u8.shape
        assert tuple(sketch_u8.shape) == (B, H, W)
        ws = self.workspace(B, H, W)
        rgb, m8 = out if out is not None else (torch.empty((B, H, W, 3), dtype=torch.uint8, device=image_u8.device),
                                               torch.empty((B, H, W), dtype=torch.uint8, device=image_u8.device))
        flags = (flags & 31) | self.exec_flags(B, H, W, low_latency, False)
        if self.lib.se_inference_u8io(self.h, self._stream(), _ptr(image_u8), _ptr(sketch_u8), _ptr(rgb), _ptr(m8), _ptr(ws),
                                      ws.numel(), B, H, W, flags):
            self._err("se_inference_u8io")
        return rgb, m8

    # ---- the demo's per-request steps (demo.py:39-73) on the device ---------------------------------------------------
    def resize_u8(self, x, size, filter=RESAMPLE_BICUBIC, out=None):
        """Pillow's Image.resize((W, H), filter) of every image of x, bit for bit (se_resize_u8): x (B,Hin,Win,C) with C in
        {1, 3}, or (B,Hin,Win) for C = 1, uint8 on the device; size = (H, W) -> the same layout at H x W."""
        import torch
        _check_dev_u8(x)
        flat = x.dim() == 3
        B, Hin, Win = x.shape[:3]
        C = 1 if flat else x.shape[3]
        H, W = size
        if out is None:
            out = torch.empty((B, H, W) if flat else (B, H, W, C), dtype=torch.uint8, device=x.device)
        _check_dev_u8(out)
        if out.numel() != B * H * W * C:
            raise SketchEditHipError("resize_u8: `out` has %d elements, expected %d" % (out.numel(), B * H * W * C))
        if self.lib.se_resize_u8(self.h, self._stream(), _ptr(x), B, Hin, Win, C, _ptr(out), H, W, int(filter)):
            self._err("se_resize_u8")
        return out

    def prepare_u8(self, image_u8, sketch_u8, H, W, out=None):
        """demo.py:40-56 for ONE request (se_prepare_u8): image_u8 (Hi,Wi,3) RGB and sketch_u8 (Hs,Ws) uint8 on the device
        (raw sizes; they may differ) -> (image (1,3,H,W), sketch (1,1,H,W)) fp32 at the working size H x W.
        `out` = (image, sketch): contiguous fp32 tensors of those sizes, e.g. one request's slot of a batch."""
        import torch
        _check_dev_u8(image_u8, sketch_u8)
        Hi, Wi = image_u8.shape[:2]
        Hs, Ws = sketch_u8.shape[:2]
        if image_u8.shape[2:] != (3,) or sketch_u8.dim() != 2:
            raise SketchEditHipError("prepare_u8: expected image (H,W,3) and sketch (H,W) uint8 arrays")
        if out is None:
            out = (torch.empty((1, 3, H, W), dtype=torch.float32, device=image_u8.device),
                   torch.empty((1, 1, H, W), dtype=torch.float32, device=image_u8.device))
        image, sketch = out
        _check_dev(image, sketch)
        if image.numel() != 3 * H * W or sketch.numel() != H * W:
            raise SketchEditHipError("prepare_u8: `out` tensors do not hold one %dx%d request" % (H, W))
        if self.lib.se_prepare_u8(self.h, self._stream(), _ptr(image_u8), Hi, Wi, _ptr(sketch_u8), Hs, Ws, _ptr(image),
                                  _ptr(sketch), H, W):
            self._err("se_prepare_u8")
        return image, sketch

    def edit_u8(self, image_u8, sketch_u8, flags, low_latency=None):
        """demo.py's process_image for B requests of one raw size as ONE library call (se_edit_u8): image_u8 (B,Hi,Wi,3),
        sketch_u8 (B,Hs,Ws) uint8 on the device -> rgb (B,Hi,Wi,3) uint8 on the device.  The working size is
        (Hi//8*8, Wi//8*8); low_latency: None = by the size of the forward (B at the working size)."""
        import torch
        _check_dev_u8(image_u8, sketch_u8)
        B, Hi, Wi, _ = image_u8.shape
        Hs, Ws = sketch_u8.shape[1:3]
        if sketch_u8.dim() != 3 or sketch_u8.shape[0] != B:
            raise SketchEditHipError("edit_u8: expected sketch (B,H,W) uint8")
        need = self.lib.se_edit_u8_workspace_bytes(self.h, B, Hi, Wi)
        if need == 0:
            self._err("se_edit_u8_workspace_bytes")
        ws = self._workspace_bytes(need)
        rgb = torch.empty((B, Hi, Wi, 3), dtype=torch.uint8, device=image_u8.device)
        flags = (flags & 31) | self.exec_flags(B, Hi // 8 * 8, Wi // 8 * 8, low_latency, False)
        if self.lib.se_edit_u8(self.h, self._stream(), _ptr(image_u8), _ptr(sketch_u8), _ptr(rgb), _ptr(ws), ws.numel(), B, Hi,
                               Wi, Hs, Ws, flags):
            self._err("se_edit_u8")
        return rgb

    # ---- editing sessions: window edits of resident frames (include/sketchedit_hip.h) -----------------------
    @staticmethod
    def _windows(frames, origins, sketches=None):
        """The se_window records of a group: frames[i] (Hi,Wi,3) uint8 on the device, origins[i] = (y0, x0), sketches[i] the
        window's (H,W) uint8 sketch on the device (gather only)."""
        n = len(frames)
        if n < 1 or len(origins) != n or (sketches is not None and len(sketches) != n):
            raise SketchEditHipError("window call: one frame, one origin (and one sketch) per request")
        wins = (Window * n)()
        for i, (f, (y0, x0)) in enumerate(zip(frames, origins)):
            _check_dev_u8(f)
            if f.dim() != 3 or f.shape[2] != 3:
                raise SketchEditHipError("window call: a frame is a (Hi,Wi,3) uint8 array")
            sk = None
            if sketches is not None:
                sk = sketches[i]
                _check_dev_u8(sk)
            wins[i] = Window(f.data_ptr(), sk.data_ptr() if sk is not None else None, f.shape[0], f.shape[1], int(y0), int(x0))
        return wins

    def _window_args(self, name, frames, origins, sketches, window_hw, H, W, locks):
        """What a window step's C entry takes after the stream, as (head, sizes): head = the records and (a locked entry:
        `locks` not None) the lock pointers; sizes = B, the window's (hs, ws) (an entry with `window_hw`; None: the window is
        (H, W)) and (H, W).  A step that reads sketches has them checked against the window's size."""
        hs, ws = (H, W) if window_hw is None else (int(v) for v in window_hw)
        head = [self._windows(frames, origins, sketches)]
        if locks is not None:
            head.append(self._locks(locks, frames))
        for sk in () if sketches is None else sketches:
            if tuple(sk.shape) != (hs, ws):
                raise SketchEditHipError("%s: a sketch is the window's %s uint8 plane"
                                         % (name, "(H,W)" if window_hw is None else "(hs,ws)"))
        return head, [len(frames)] + ([] if window_hw is None else [hs, ws]) + [H, W]

    def _window_gather(self, fn, name, frames, origins, sketches, window_hw, H, W):
        """the one body of window_gather_u8 and window_gather_resize_u8: `fn` = the entry's C function, `name` its name"""
        import torch
        head, sizes = self._window_args(name, frames, origins, sketches, window_hw, H, W, None)
        B, dev = len(frames), frames[0].device
        image = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        sketch = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        if fn(self.h, self._stream(), *head, *sizes, _ptr(image), _ptr(sketch)):
            self._err("se_" + name)
        return image, sketch

    def _window_paste(self, fn, name, frames, origins, window_hw, rgb, mask_u8, locks):
        """the one body of the three pastes; `locks` None for the two entries that take none"""
        _check_dev_u8(rgb, mask_u8)
        B, H, W = mask_u8.shape
        if tuple(rgb.shape) != (B, H, W, 3) or len(frames) != B:
            raise SketchEditHipError("%s: expected rgb (B,H,W,3), mask_u8 (B,H,W) and one frame per request" % name)
        head, sizes = self._window_args(name, frames, origins, None, window_hw, H, W, locks)
        if fn(self.h, self._stream(), *head, *sizes, _ptr(rgb), _ptr(mask_u8)):
            self._err("se_" + name)

    def _edit_window(self, fns, name, frames, origins, sketches, window_hw, H, W, locks, flags, commit, low_latency):
        """the one body of the three edit_window*_u8: `fns` = (the entry's C function, its workspace query) -- each entry
        keeps its own pair, their workspaces differ"""
        import torch
        fn, workspace_bytes = fns
        head, sizes = self._window_args(name, frames, origins, sketches, window_hw, H, W, locks)
        B, dev = len(frames), frames[0].device
        need = workspace_bytes(self.h, *sizes)
        if need == 0:
            self._err("se_%s_workspace_bytes" % name)
        ws = self._workspace_bytes(need)
        rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        m8 = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        hits = torch.empty((B, 4), dtype=torch.int32, device=dev)
        flags = (flags & 31) | self.exec_flags(B, H, W, low_latency, False)
        if fn(self.h, self._stream(), *head, *sizes, _ptr(rgb), _ptr(m8), _ptr(hits), 1 if commit else 0, _ptr(ws), ws.numel(), flags):
            self._err("se_" + name)
        return rgb, m8, hits

    def window_gather_u8(self, frames, origins, sketches, H, W):
        """se_window_gather_u8: the H x W window at origins[i] = (y0, x0) of every frame and its sketch -> the forward's inputs
        (image (B,3,H,W), sketch (B,1,H,W)) fp32, bit-identical to dequantize_u8 of the contiguous crops.  One launch."""
        return self._window_gather(self.lib.se_window_gather_u8, "window_gather_u8", frames, origins, sketches, None, H, W)

    def window_border_u8(self, frames, origins, mask_u8):
        """se_window_border_u8: mask_u8 (B,H,W) uint8 -> (B,4) int32 on the device: pixels >= 128 on the top / bottom / left /
        right edge of each window; a side on its frame's own edge counts 0."""
        import torch
        _check_dev_u8(mask_u8)
        B, H, W = mask_u8.shape
        wins = self._windows(frames, origins)
        if len(frames) != B:
            raise SketchEditHipError("window_border_u8: one frame per mask")
        hits = torch.empty((B, 4), dtype=torch.int32, device=mask_u8.device)
        if self.lib.se_window_border_u8(self.h, self._stream(), wins, B, H, W, _ptr(mask_u8), _ptr(hits)):
            self._err("se_window_border_u8")
        return hits

    def window_paste_u8(self, frames, origins, rgb, mask_u8):
        """se_window_paste_u8, in place: frames[i][y0 + y, x0 + x] = rgb[i, y, x] where mask_u8[i, y, x] > 0; rgb (B,H,W,3),
        mask_u8 (B,H,W) uint8 on the device.  Overlapping windows of one frame in one call are refused."""
        self._window_paste(self.lib.se_window_paste_u8, "window_paste_u8", frames, origins, None, rgb, mask_u8, None)

    def edit_window_u8(self, frames, origins, sketches, H, W, flags, commit=True, low_latency=None):
        """se_edit_window_u8: gather, the forward with fused quantisation, the border counts and (commit) the paste into the
        frames, as ONE library call without a host synchronisation.  -> (rgb (B,H,W,3) uint8, mask_u8 (B,H,W) uint8,
        hits (B,4) int32), on the device.  low_latency: None = by the size of the forward, (B, H, W) of the WINDOW."""
        return self._edit_window((self.lib.se_edit_window_u8, self.lib.se_edit_window_u8_workspace_bytes), "edit_window_u8",
                                 frames, origins, sketches, None, H, W, None, flags, commit, low_latency)

    # ---- the same at a working size: window (hs, ws) in the frame, forward at (H, W) --------------------------
    def window_gather_resize_u8(self, frames, origins, sketches, window_hw, H, W):
        """se_window_gather_resize_u8: the hs x ws window at origins[i] of every frame and its (hs, ws) sketch, resampled
        (Pillow's BICUBIC, bit for bit) into the forward's inputs at H x W -> (image (B,3,H,W), sketch (B,1,H,W)) fp32:
        prepare_u8 of the contiguous crops, without the crops."""
        return self._window_gather(self.lib.se_window_gather_resize_u8, "window_gather_resize_u8", frames, origins, sketches,
                                   window_hw, H, W)

    def window_paste_resize_u8(self, frames, origins, window_hw, rgb, mask_u8):
        """se_window_paste_resize_u8, in place: rgb (B,H,W,3) and mask_u8 (B,H,W) at the working size are resampled to the
        hs x ws windows (BICUBIC, both) and frames[i][y0 + y, x0 + x] takes the resampled colour where the resampled mask
        byte is > 0.  Overlapping windows of one frame in one call are refused."""
        self._window_paste(self.lib.se_window_paste_resize_u8, "window_paste_resize_u8", frames, origins, window_hw, rgb, mask_u8,
                           None)

    def edit_window_scaled_u8(self, frames, origins, sketches, window_hw, H, W, flags, commit=True, low_latency=None):
        """se_edit_window_scaled_u8: the window edit with the forward at the working size H x W, ONE library call without a
        host synchronisation.  -> (rgb (B,H,W,3) uint8, mask_u8 (B,H,W) uint8, hits (B,4) int32) on the device, rgb and
        mask_u8 AT THE WORKING SIZE.  low_latency: None = by the size of the forward, (B, H, W)."""
        return self._edit_window((self.lib.se_edit_window_scaled_u8, self.lib.se_edit_window_scaled_u8_workspace_bytes),
                                 "edit_window_scaled_u8", frames, origins, sketches, window_hw, H, W, None, flags, commit, low_latency)

    # ---- the undo journal of a session ------------------------------------------------------------------------
    @staticmethod
    def window_saved_bytes(hs, ws):
        """se_window_saved_bytes: the bytes of one journal slot, hs rows of round_up(3 ws, 16); 0 if hs or ws < 16 (host only)"""
        return int(load_library().se_window_saved_bytes(int(hs), int(ws)))

    def _journal(self, fn, name, frames, origins, window_hw, slots):
        hs, ws = (int(v) for v in window_hw)
        wins = self._windows(frames, origins)
        need = self.window_saved_bytes(hs, ws)
        if len(slots) != len(frames):
            raise SketchEditHipError("%s: one slot per request" % name)
        for t in slots:
            _check_dev_u8(t)
            if need and t.numel() < need:
                raise SketchEditHipError("%s: a slot holds window_saved_bytes(hs, ws) = %d bytes" % (name, need))
        ptrs = (ctypes.c_void_p * len(slots))(*[t.data_ptr() for t in slots])
        if fn(self.h, self._stream(), wins, len(frames), hs, ws, ptrs):
            self._err(name)

    def window_save_u8(self, frames, origins, window_hw):
        """se_window_save_u8: the hs x ws rectangle at origins[i] of every frame -> a new slot per request, (hs, pitch) uint8
        with pitch = round_up(3 ws, 16) (a row's first 3 ws bytes are the crop's row).  One launch.  -> [slot tensors]"""
        import torch
        hs, ws = (int(v) for v in window_hw)
        n = self.window_saved_bytes(hs, ws)                   # (0: a window the library refuses; it says why)
        slots = [torch.empty(n, dtype=torch.uint8, device=f.device).view(hs, n // hs) if n else
                 torch.empty(16, dtype=torch.uint8, device=f.device) for f in frames]
        self._journal(self.lib.se_window_save_u8, "se_window_save_u8", frames, origins, (hs, ws), slots)
        return slots

    def window_swap_u8(self, frames, origins, window_hw, slots):
        """se_window_swap_u8, in place: the hs x ws rectangle at origins[i] of frames[i] <-> slots[i] (as window_save_u8 made
        it).  Overlapping windows of one frame in one call are refused."""
        self._journal(self.lib.se_window_swap_u8, "se_window_swap_u8", frames, origins, window_hw, slots)

    # ---- locked regions of a session: locks[i] = the (Hi,Wi) uint8 plane of frames[i] on the device, or None --
    @staticmethod
    def _locks(locks, frames):
        if len(locks) != len(frames):
            raise SketchEditHipError("locked window call: one lock plane (or None) per request")
        for t, f in zip(locks, frames):
            if t is not None:
                _check_dev_u8(t)
                if tuple(t.shape) != tuple(f.shape[:2]):
                    raise SketchEditHipError("locked window call: a lock plane is the frame's (Hi,Wi) uint8 plane")
        return (ctypes.c_void_p * len(locks))(*[None if t is None else t.data_ptr() for t in locks])

    def window_gather_lock_u8(self, frames, origins, locks, window_hw, H, W):
        """se_window_gather_lock_u8: the hs x ws window at origins[i] of every lock plane -> (B,H,W) uint8 in {0,1} at the
        working size H x W: `crop > 0` when unscaled, else Pillow's BICUBIC resize of the crop, `> 0`.  None -> zeros."""
        import torch
        hs, ws = (int(v) for v in window_hw)
        wins = self._windows(frames, origins)
        ptrs = self._locks(locks, frames)
        out = torch.empty((len(frames), H, W), dtype=torch.uint8, device=frames[0].device)
        if self.lib.se_window_gather_lock_u8(self.h, self._stream(), wins, ptrs, len(frames), hs, ws, H, W, _ptr(out)):
            self._err("se_window_gather_lock_u8")
        return out

    def window_paste_locked_u8(self, frames, origins, locks, window_hw, rgb, mask_u8):
        """se_window_paste_locked_u8, in place: window_paste_resize_u8 (window_paste_u8 when the sizes agree) that leaves
        every pixel whose byte of its frame's lock plane is non-zero untouched, whatever the mask says."""
        self._window_paste(self.lib.se_window_paste_locked_u8, "window_paste_locked_u8", frames, origins, window_hw, rgb, mask_u8,
                           locks)

    def edit_window_locked_u8(self, frames, origins, sketches, locks, window_hw, H, W, flags, commit=True, low_latency=None):
        """se_edit_window_locked_u8: edit_window_scaled_u8 (edit_window_u8 when (H, W) == window_hw) in which no edit changes
        a locked pixel: the lock enters the forward (inference_u8(lock=)) and the paste.  -> (rgb, mask_u8, hits) as there."""
        return self._edit_window((self.lib.se_edit_window_locked_u8, self.lib.se_edit_window_locked_u8_workspace_bytes),
                                 "edit_window_locked_u8", frames, origins, sketches, window_hw, H, W, locks, flags, commit, low_latency)

    # ---- the feathered paste -------------------------------------------------------------------------------------
    def window_paste_feather_u8(self, frames, origins, locks, window_hw, radius, rgb, m8):
        """se_window_paste_feather_u8, in place: rgb (B,hs,ws,3) and m8 (B,hs,ws) uint8 on the device AT THE WINDOW'S SIZE
        window_hw = (hs, ws) (any sides >= 16) are blended into frames[i] at origins[i] = (y0, x0) by the rule of
        include/sketchedit_feather.h: a selected pixel (m8 > 0, not locked) takes c / n of rgb and (n - c) / n of the frame,
        c = the selected pixels in the (2 radius + 1)^2 box around it; radius 0 .. 16, 0 = window_paste_locked_u8.  locks:
        one (Hi,Wi) uint8 plane or None per request, or None for none.  One launch; overlapping windows of one frame are
        refused."""
        _check_dev_u8(rgb, m8)
        hs, ws = (int(v) for v in window_hw)
        B = len(frames)
        if tuple(m8.shape) != (B, hs, ws) or tuple(rgb.shape) != (B, hs, ws, 3):
            raise SketchEditHipError("window_paste_feather_u8: expected rgb (B,hs,ws,3), m8 (B,hs,ws) at the window's size and one "
                                     "frame per request")
        wins = self._windows(frames, origins)
        ptrs = None if locks is None else self._locks(locks, frames)
        if self.lib.se_window_paste_feather_u8(self.h, self._stream(), wins, ptrs, B, hs, ws, int(radius), _ptr(rgb), _ptr(m8)):
            self._err("se_window_paste_feather_u8")

    # ---- fills of a painted region (include/sketchedit_fill.h) ------------------------------------------------------
    def fill(self, image, hole, flags, sketch=None, lock=None, visualize=False, low_latency=None):
        """se_fill: netG alone on a hole the caller gives.  image (B,3,H,W) fp32, hole (B,H,W) uint8 on the device, non-zero =
        fill; sketch (B,1,H,W) fp32 or None (zeros); lock (B,H,W) uint8 or None -- a locked pixel is never a hole.
        -> dict(composed[, coarse, fine, hard]) with hole = fill & ~lock in `hard`: coarse, fine = netG(image, image, hard,
        hard, sketch) and composed = where(hard, fine, image), bit for bit.  low_latency as `inference`."""
        import torch
        _check_dev(image, sketch)
        B, _, H, W = image.shape
        for name, t in (("hole", hole), ("lock", lock)):
            if t is not None or name == "hole":
                _check_dev_u8(t)
                if tuple(t.shape) != (B, H, W):
                    raise SketchEditHipError("%s: expected a (B,H,W) uint8 plane of the images' size" % name)
        if sketch is not None and tuple(sketch.shape) != (B, 1, H, W):
            raise SketchEditHipError("sketch: expected a (B,1,H,W) tensor of the images' size")
        ws = self.workspace(B, H, W)
        mk = lambda c: torch.empty((B, c, H, W), dtype=torch.float32, device=image.device)     # noqa: E731
        r = dict(composed=mk(3))
        if visualize:
            r.update(coarse=mk(3), fine=mk(3), hard=mk(1))
        flags = (flags & 31) | self.exec_flags(B, H, W, low_latency, False)
        if self.lib.se_fill(self.h, self._stream(), _ptr(image), _ptr(sketch), _ptr(hole), _ptr(lock), _ptr(r["composed"]),
                            _ptr(r.get("coarse")), _ptr(r.get("fine")), _ptr(r.get("hard")), _ptr(ws), ws.numel() // 16 * 16, B, H, W, flags):
            self._err("se_fill")
        return r

    @staticmethod
    def _planes(planes, frames, what, required):
        """the HOST array of a fill call's plane pointers: one (Hi,Wi) uint8 plane per request (or None unless `required`)"""
        if len(planes) != len(frames):
            raise SketchEditHipError("fill call: one %s plane per request" % what)
        for t, f in zip(planes, frames):
            if t is None and not required:
                continue
            _check_dev_u8(t)
            if tuple(t.shape) != tuple(f.shape[:2]):
                raise SketchEditHipError("fill call: a %s plane is the frame's (Hi,Wi) uint8 plane" % what)
        return (ctypes.c_void_p * len(planes))(*[None if t is None else t.data_ptr() for t in planes])

    def fill_window_u8(self, frames, origins, sketches, holes, locks, window_hw, H, W, flags, low_latency=None, raw=False):
        """se_fill_window_u8: the fill of the (hs, ws) windows at origins[i] of resident frames with the forward at H x W (equal:
        the frame's own resolution), ONE library call.  holes[i]: the frame's (Hi,Wi) uint8 fill plane on the device, non-zero
        = fill; locks: a plane or None per request, or None; sketches: the window's (hs,ws) uint8 sketch or None per request,
        or None.  Never commits.  -> (rgb (B,H,W,3), mask_u8 (B,H,W)) on the device, mask_u8 255 in the hole: what the pastes
        take, with the keep planes of fill_keep_u8 in place of the locks.  raw (SE_FLAG_RAW_FINE): rgb is the quantisation of
        netG's `fine` at every pixel, not of the composite -- equal in the hole, the generator's own prediction on its rim,
        which is what a seamless paste (move_blend_u8) reads there; mask_u8 is the same."""
        import torch
        hs, ws = (int(v) for v in window_hw)
        B, dev = len(frames), frames[0].device if frames else None
        wins = self._windows(frames, origins)
        if sketches is not None:
            if len(sketches) != B:
                raise SketchEditHipError("fill_window_u8: one sketch (or None) per request")
            for i, sk in enumerate(sketches):
                if sk is None:
                    continue
                _check_dev_u8(sk)
                if tuple(sk.shape) != (hs, ws):
                    raise SketchEditHipError("fill_window_u8: a sketch is the window's (hs,ws) uint8 plane")
                wins[i].sketch_u8 = sk.data_ptr()
        hp = self._planes(holes, frames, "fill", True)
        lp = None if locks is None else self._planes(locks, frames, "lock", False)
        need = self.lib.se_fill_window_u8_workspace_bytes(self.h, B, hs, ws, H, W)
        if need == 0:
            self._err("se_fill_window_u8_workspace_bytes")
        wsp = self._workspace_bytes(need)
        rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        m8 = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        flags = (flags & 31) | self.exec_flags(B, H, W, low_latency, False) | (FLAG_RAW_FINE if raw else 0)
        if self.lib.se_fill_window_u8(self.h, self._stream(), wins, hp, lp, B, hs, ws, H, W, _ptr(rgb), _ptr(m8), _ptr(wsp),
                                      wsp.numel() // 16 * 16, flags):
            self._err("se_fill_window_u8")
        return rgb, m8

    def fill_keep_u8(self, frames, origins, holes, locks, window_hw, keeps=None):
        """se_fill_keep_u8: the keep planes of a fill's paste -- the (hs, ws) rectangle at origins[i] of keeps[i], an (Hi,Wi)
        uint8 plane on the device, becomes 255 where holes[i] is 0 or locks[i] is non-zero, else 0; no other byte is written.
        keeps None: new planes, whose bytes outside the rectangle are undefined (the pastes read none of them).  -> keeps"""
        import torch
        hs, ws = (int(v) for v in window_hw)
        wins = self._windows(frames, origins)
        hp = self._planes(holes, frames, "fill", True)
        lp = None if locks is None else self._planes(locks, frames, "lock", False)
        if keeps is None:
            keeps = [torch.empty(tuple(f.shape[:2]), dtype=torch.uint8, device=f.device) for f in frames]
        kp = self._planes(keeps, frames, "keep", True)
        if self.lib.se_fill_keep_u8(self.h, self._stream(), wins, hp, lp, kp, len(frames), hs, ws):
            self._err("se_fill_keep_u8")
        return keeps

    # ---- selection by colour (include/sketchedit_select.h) ----------------------------------------------------------
    @staticmethod
    def _state_plane(t, what):
        _check_dev_u8(t)
        if t.dim() != 2:
            raise SketchEditHipError("%s: an (Hi,Wi) uint8 plane on the device" % what)
        return int(t.shape[0]), int(t.shape[1])

    def select_similar_u8(self, frame, seed, tolerance, contiguous, state=None):
        """se_select_similar_u8: frame (Hi,Wi,3) uint8 on the device, seed = (y, x) -> the state plane (Hi,Wi) uint8 there: 255 at
        the seed; elsewhere, where max_c |frame[y, x, c] - frame[seed, c]| <= tolerance, 1 if `contiguous` else 255; 0 for every
        other pixel.  `state`: a plane of that shape to write into, any alignment (every byte is written)."""
        import torch
        _check_dev_u8(frame)
        if frame.dim() != 3 or frame.shape[2] != 3:
            raise SketchEditHipError("select_similar_u8: a frame is an (Hi,Wi,3) uint8 tensor")
        Hi, Wi = int(frame.shape[0]), int(frame.shape[1])
        if state is None:
            state = torch.empty((Hi, Wi), dtype=torch.uint8, device=frame.device)
        if self._state_plane(state, "select_similar_u8: state") != (Hi, Wi):
            raise SketchEditHipError("select_similar_u8: the state plane is the frame's (Hi,Wi) plane")
        if self.lib.se_select_similar_u8(self.h, self._stream(), _ptr(frame), Hi, Wi, int(seed[0]), int(seed[1]), int(tolerance),
                                         1 if contiguous else 0, _ptr(state)):
            self._err("se_select_similar_u8")
        return state

    def select_flood_u8(self, state, passes=8, changed=None):
        """se_select_flood_u8: `passes` (1 .. 64) passes over the state plane, in place: a byte of 1 next to a reached byte
        becomes 255, closed over every 64 x 64 tile.  -> `changed`, (passes,) int32 on the device (`changed`: a tensor of that
        shape to write into): 1 where that pass stored a byte, else 0.  A 0 says the plane is at its fixed point."""
        import torch
        Hi, Wi = self._state_plane(state, "select_flood_u8: state")
        passes = int(passes)
        if changed is None and passes > 0:
            changed = torch.empty((passes,), dtype=torch.int32, device=state.device)
        if changed is not None and not (isinstance(changed, torch.Tensor) and changed.is_cuda and changed.dtype == torch.int32
                                        and changed.is_contiguous() and changed.numel() == passes):
            raise SketchEditHipError("select_flood_u8: changed is a contiguous (passes,) int32 CUDA(HIP) tensor")
        if self.lib.se_select_flood_u8(self.h, self._stream(), _ptr(state), Hi, Wi, passes, _ptr(changed)):
            self._err("se_select_flood_u8")
        return changed

    def select_grow_u8(self, state, grow, out=None):
        """se_select_grow_u8: the state plane -> a fill plane (Hi,Wi) uint8 on the device (`out`: another plane of that shape,
        any alignment; every byte is written): 255 where a byte of 255 lies within Chebyshev distance `grow` (0 .. 16), else 0."""
        import torch
        Hi, Wi = self._state_plane(state, "select_grow_u8: state")
        if out is None:
            out = torch.empty((Hi, Wi), dtype=torch.uint8, device=state.device)
        if self._state_plane(out, "select_grow_u8: out") != (Hi, Wi):
            raise SketchEditHipError("select_grow_u8: out is a plane of the state's shape")
        if self.lib.se_select_grow_u8(self.h, self._stream(), _ptr(state), Hi, Wi, int(grow), _ptr(out)):
            self._err("se_select_grow_u8")
        return out

    # ---- lasso selections and their algebra (include/sketchedit_lasso.h) ---------------------------------------------
    def lasso_fill_u8(self, edges, Hi, Wi, out=None):
        """se_lasso_fill_u8: `edges` (N,4) int32 on the device, [ax, ay, bx, by] in quarter pixels of an (Hi,Wi) frame, N >= 0 ->
        the fill plane (Hi,Wi) uint8 there: 255 where an odd number of edges cross the pixel's scanline strictly left of its
        centre (the even-odd rule of the header), else 0.  `out`: a plane of that shape to write into, any alignment (every byte
        is written)."""
        import torch
        if not (isinstance(edges, torch.Tensor) and edges.is_cuda and edges.dtype == torch.int32 and edges.is_contiguous()
                and edges.dim() == 2 and edges.shape[1] == 4):
            raise SketchEditHipError("lasso_fill_u8: edges are an (N,4) contiguous int32 CUDA(HIP) tensor")
        Hi, Wi, N = int(Hi), int(Wi), int(edges.shape[0])
        if out is None:
            if Hi < 1 or Wi < 1:
                raise SketchEditHipError("lasso_fill_u8: bad Hi=%d Wi=%d" % (Hi, Wi))
            out = torch.empty((Hi, Wi), dtype=torch.uint8, device=edges.device)
        if self._state_plane(out, "lasso_fill_u8: out") != (Hi, Wi):
            raise SketchEditHipError("lasso_fill_u8: out is an (Hi,Wi) plane")
        if self.lib.se_lasso_fill_u8(self.h, self._stream(), _ptr(edges) if N else None, N, Hi, Wi, _ptr(out)):
            self._err("se_lasso_fill_u8")
        return out

    def plane_combine_u8(self, a, b, op, out=None):
        """se_plane_combine_u8: planes (Hi,Wi) uint8 on the device, non-zero = selected -> `out` (a new plane, or a plane of that
        shape: `a` itself, `b` itself, or one that shares no byte with them; any alignment), 0 / 255: op COMBINE_ADD a | b,
        COMBINE_SUBTRACT a & ~b, COMBINE_INTERSECT a & b, COMBINE_XOR a ^ b, COMBINE_INVERT ~a (b is None)."""
        import torch
        Hi, Wi = self._state_plane(a, "plane_combine_u8: a")
        if b is not None and self._state_plane(b, "plane_combine_u8: b") != (Hi, Wi):
            raise SketchEditHipError("plane_combine_u8: b is a plane of a's shape")
        if out is None:
            out = torch.empty((Hi, Wi), dtype=torch.uint8, device=a.device)
        if self._state_plane(out, "plane_combine_u8: out") != (Hi, Wi):
            raise SketchEditHipError("plane_combine_u8: out is a plane of a's shape")
        if self.lib.se_plane_combine_u8(self.h, self._stream(), _ptr(a), _ptr(b), Hi, Wi, int(op), _ptr(out)):
            self._err("se_plane_combine_u8")
        return out

    # ---- modify a selection's shape (include/sketchedit_modify.h) ----------------------------------------------------
    def plane_modify_u8(self, plane, op, radius, out=None):
        """se_plane_modify_u8: a plane (Hi,Wi) uint8 on the device, non-zero = selected -> `out` (a NEW plane, or another plane of
        that shape that shares no byte with it; any alignment; every byte is written), 0 / 255: op MODIFY_EXPAND the pixels
        within the disc of `radius` (1 .. 32) of a selected one, MODIFY_CONTRACT the selected pixels with no unselected pixel
        of the frame in their disc, MODIFY_SMOOTH the majority vote in the disc (a tie keeps the pixel).  One launch."""
        import torch
        Hi, Wi = self._state_plane(plane, "plane_modify_u8: plane")
        if out is None:
            out = torch.empty((Hi, Wi), dtype=torch.uint8, device=plane.device)
        if self._state_plane(out, "plane_modify_u8: out") != (Hi, Wi):
            raise SketchEditHipError("plane_modify_u8: out is a plane of the plane's shape")
        if self.lib.se_plane_modify_u8(self.h, self._stream(), _ptr(plane), Hi, Wi, int(op), int(radius), _ptr(out)):
            self._err("se_plane_modify_u8")
        return out

    # ---- the outline of a selection (include/sketchedit_outline.h) ------------------------------------------------------
    def outline_u8(self, plane, cap):
        """se_outline_u8: a plane (Hi,Wi) uint8 on the device, non-zero = selected -> ONE int32 tensor of 2 + 4 cap words there:
        [total, written], then the first written = min(total, cap) boundary records [ax, ay, bx, by] in quarter pixels, in the
        header's order (a valid `edges` argument of lasso_fill_u8 once reshaped to (-1, 4)); the words behind the written
        records are not written.  One download gives a caller everything.  cap: 0 .. OUTLINE_MAX_CAP."""
        import torch
        Hi, Wi = self._state_plane(plane, "outline_u8: plane")
        if not isinstance(cap, (int, np.integer)) or isinstance(cap, (bool, np.bool_)) or not 0 <= cap <= OUTLINE_MAX_CAP:
            raise SketchEditHipError("outline_u8: cap is an int 0 .. %d (got %r)" % (OUTLINE_MAX_CAP, cap))
        cap = int(cap)
        out = torch.empty((2 + 4 * cap,), dtype=torch.int32, device=plane.device)
        need = self.lib.se_outline_u8_workspace_bytes(self.h, Hi, Wi)
        if need == 0:
            self._err("se_outline_u8_workspace_bytes")
        ws_t = self._workspace_bytes(need)
        edges = ctypes.c_void_p(out.data_ptr() + 8) if cap else None
        if self.lib.se_outline_u8(self.h, self._stream(), _ptr(plane), Hi, Wi, edges, cap, _ptr(out), _ptr(ws_t), ws_t.numel()):
            self._err("se_outline_u8")
        return out

    # ---- move or clone a selection (include/sketchedit_move.h) -------------------------------------------------------
    def _lift_args(self, what, frame, lift, lift_rect, sel, lock, box):
        """the checks every entry that takes a lift shares -> (Hi, Wi, lift rectangle, box) as ints"""
        _check_dev_u8(frame)
        if frame.dim() != 3 or frame.shape[2] != 3:
            raise SketchEditHipError("%s: a frame is an (Hi,Wi,3) uint8 tensor" % what)
        Hi, Wi = int(frame.shape[0]), int(frame.shape[1])
        if self._state_plane(sel, what + ": sel") != (Hi, Wi) or (lock is not None and self._state_plane(lock, what + ": lock") != (Hi, Wi)):
            raise SketchEditHipError("%s: sel and lock are the frame's (Hi,Wi) planes" % what)
        lr = tuple(int(v) for v in lift_rect)
        _check_dev_u8(lift)
        need = self.window_saved_bytes(lr[2], lr[3])
        if need and lift.numel() < need:
            raise SketchEditHipError("%s: a lift holds window_saved_bytes(lh, lw) = %d bytes" % (what, need))
        return Hi, Wi, lr, tuple(int(v) for v in box)

    def move_drop_u8(self, frame, lift, lift_rect, sel, lock, box, offset, flip=0, radius=0):
        """se_move_drop_u8, in place on `frame` (Hi,Wi,3) uint8 on the device: the pixels of `box` = (by0, bx0, by1, bx1) that
        `sel` (an (Hi,Wi) plane, non-zero = selected) selects, as `lift` holds them -- the journal slot window_save_u8 made of
        `lift_rect` = (ly0, lx0, lh, lw), a rectangle that holds the box -- land `offset` = (dy, dx) away, mirrored about the box
        by `flip` (MOVE_FLIP_X | MOVE_FLIP_Y), where `lock` (a plane or None) is 0; `radius` 0 .. 16 fades their rim into the
        frame.  No other byte changes.  One launch; none when the whole box lands outside the frame."""
        Hi, Wi, (ly0, lx0, lh, lw), (by0, bx0, by1, bx1) = self._lift_args("move_drop_u8", frame, lift, lift_rect, sel, lock, box)
        if self.lib.se_move_drop_u8(self.h, self._stream(), _ptr(frame), Hi, Wi, _ptr(lift), ly0, lx0, lh, lw, _ptr(sel), _ptr(lock),
                                    by0, bx0, by1, bx1, int(offset[0]), int(offset[1]), int(flip), int(radius)):
            self._err("se_move_drop_u8")

    def move_blend_u8(self, frame, lift, lift_rect, sel, lock, box, offset, flip=0):
        """se_move_blend_u8 (include/sketchedit_blend.h), in place on `frame`: move_drop_u8's arguments without the
        radius; the object keeps its own detail and takes the local colour of the place it lands in -- the lift's bytes plus a
        membrane that equals frame - lift on the object's rim, made by a fixed schedule of integer steps.  `lift_rect` should
        hold the box grown by one pixel (the rim's sources); a side of the box is at most BLEND_MAX_SIDE.  The launches depend
        on the box's size alone; none when the whole box lands outside the frame."""
        Hi, Wi, (ly0, lx0, lh, lw), (by0, bx0, by1, bx1) = self._lift_args("move_blend_u8", frame, lift, lift_rect, sel, lock, box)
        need = self.lib.se_move_blend_u8_workspace_bytes(by1 - by0, bx1 - bx0)
        if need == 0:
            raise SketchEditHipError("move_blend_u8: a side of the box %r is outside 1 .. %d" % ((by0, bx0, by1, bx1), BLEND_MAX_SIDE))
        ws_t = self._workspace_bytes(need)
        if self.lib.se_move_blend_u8(self.h, self._stream(), _ptr(frame), Hi, Wi, _ptr(lift), ly0, lx0, lh, lw, _ptr(sel), _ptr(lock),
                                     by0, bx0, by1, bx1, int(offset[0]), int(offset[1]), int(flip), _ptr(ws_t), ws_t.numel()):
            self._err("se_move_blend_u8")

    def plane_shift_u8(self, sel, box, offset, flip=0, out=None):
        """se_plane_shift_u8: `sel` (Hi,Wi) uint8 on the device, non-zero = selected -> `out` (a new plane, or another plane of
        that shape at any alignment; every byte is written), 0 / 255: the selected pixels of `box` = (by0, bx0, by1, bx1) moved by
        `offset` = (dy, dx) and mirrored about the box by `flip`; what leaves the frame is dropped."""
        import torch
        Hi, Wi = self._state_plane(sel, "plane_shift_u8: sel")
        if out is None:
            out = torch.empty((Hi, Wi), dtype=torch.uint8, device=sel.device)
        if self._state_plane(out, "plane_shift_u8: out") != (Hi, Wi):
            raise SketchEditHipError("plane_shift_u8: out is a plane of sel's shape")
        by0, bx0, by1, bx1 = (int(v) for v in box)
        if self.lib.se_plane_shift_u8(self.h, self._stream(), _ptr(sel), Hi, Wi, by0, bx0, by1, bx1, int(offset[0]), int(offset[1]), int(flip),
                                      _ptr(out)):
            self._err("se_plane_shift_u8")
        return out

    # ---- the canvas of a session (include/sketchedit_canvas.h) ---------------------------------------------------------
    def canvas_u8(self, src, out_hw, origin=(0, 0), orient=0, pad=CANVAS_EDGE, pad_rgb=0, src_hw=None, out=None, device=None):
        """se_canvas_u8: `src` (Hi,Wi,3) or (Hi,Wi) uint8 on the device -> `out` (a NEW tensor (Hn,Wn,3) / (Hn,Wn), or one of
        that shape that shares no byte with src; any alignment; every byte is written): the rectangle of `out_hw` = (Hn, Wn) at
        `origin` = (oy, ox) of src oriented by `orient` (0 .. 7: CANVAS_MIRROR_X | CANVAS_MIRROR_Y | CANVAS_TRANSPOSE, the
        transpose last), what lies outside filled by `pad` (CANVAS_EDGE, CANVAS_REFLECT, or CANVAS_CONSTANT with the colour
        `pad_rgb`, byte c of a pixel = (pad_rgb >> 8 c) & 255).  src None: a plane of zeros of `src_hw` that is never read --
        with CANVAS_CONSTANT 255 the plane of the NEW area.  One launch."""
        import torch
        Hn, Wn = (int(v) for v in out_hw)
        if src is None:
            if src_hw is None:
                raise SketchEditHipError("canvas_u8: without src, src_hw = (Hi, Wi) says what the rectangle is taken of")
            Hi, Wi, C = int(src_hw[0]), int(src_hw[1]), 1
            dev = out.device if out is not None else (device if device is not None else torch.device("cuda", self.device))
        else:
            _check_dev_u8(src)
            if not (src.dim() == 2 or (src.dim() == 3 and src.shape[2] == 3)):
                raise SketchEditHipError("canvas_u8: src is an (Hi,Wi,3) frame or an (Hi,Wi) plane")
            Hi, Wi, C = int(src.shape[0]), int(src.shape[1]), 1 if src.dim() == 2 else 3
            dev = src.device
        shape = (Hn, Wn) if C == 1 else (Hn, Wn, 3)
        if out is None:
            if not (1 <= Hn <= CANVAS_MAX_SIDE and 1 <= Wn <= CANVAS_MAX_SIDE and C * Hn * Wn < 1 << 31):
                raise SketchEditHipError("canvas_u8: bad out_hw=%r (sides 1 .. %d, C Hn Wn < 2^31)" % ((Hn, Wn), CANVAS_MAX_SIDE))
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        _check_dev_u8(out)
        if tuple(out.shape) != shape:
            raise SketchEditHipError("canvas_u8: out is a uint8 tensor of shape %r" % (shape,))
        if self.lib.se_canvas_u8(self.h, self._stream(), _ptr(src), Hi, Wi, C, _ptr(out), Hn, Wn, int(origin[0]), int(origin[1]),
                                     int(orient), int(pad), int(pad_rgb) & 0xffffffff):
            self._err("se_canvas_u8")
        return out

    # ---- scale and rotate a selection (include/sketchedit_warp.h) ------------------------------------------------------
    @staticmethod
    def _warp_map(m, what):
        """the six Q16 ints of an inverse map -> a host array of six long long"""
        try:
            vals = [int(v) for v in m]
        except (TypeError, ValueError):
            vals = []
        if len(vals) != 6 or any(abs(v) >= 1 << 63 for v in vals):
            raise SketchEditHipError("%s: m is six ints (ayy, ayx, ay0, axy, axx, ax0) in Q16" % what)
        return (ctypes.c_longlong * 6)(*vals)

    def warp_drop_u8(self, frame, lift, lift_rect, sel, lock, box, rect, m):
        """se_warp_drop_u8, in place on `frame` (Hi,Wi,3) uint8 on the device: the pixels of `box` = (by0, bx0, by1, bx1) that
        `sel` (an (Hi,Wi) plane, non-zero = selected) selects, as `lift` holds them -- the journal slot window_save_u8 made of
        `lift_rect` = (ly0, lx0, lh, lw), a rectangle that holds the box -- gathered through the inverse map `m` (six Q16 ints)
        with bilinear taps and blended by their coverage into `rect` = (ry0, rx0, rh, rw) of the frame where `lock` (a plane or
        None) is 0.  No other byte changes.  One launch."""
        Hi, Wi, (ly0, lx0, lh, lw), (by0, bx0, by1, bx1) = self._lift_args("warp_drop_u8", frame, lift, lift_rect, sel, lock, box)
        ry0, rx0, rh, rw = (int(v) for v in rect)
        mm = self._warp_map(m, "warp_drop_u8")
        if self.lib.se_warp_drop_u8(self.h, self._stream(), _ptr(frame), Hi, Wi, _ptr(lift), ly0, lx0, lh, lw, _ptr(sel), _ptr(lock),
                                    by0, bx0, by1, bx1, ry0, rx0, rh, rw, mm):
            self._err("se_warp_drop_u8")

    def plane_warp_u8(self, sel, box, m, out=None):
        """se_plane_warp_u8: `sel` (Hi,Wi) uint8 on the device, non-zero = selected -> `out` (a new plane, or another plane of
        that shape at any alignment; every byte is written), 255 where the selected pixels of `box` = (by0, bx0, by1, bx1),
        gathered through the inverse map `m` as warp_drop_u8 gathers them, cover at least half a pixel, else 0."""
        import torch
        Hi, Wi = self._state_plane(sel, "plane_warp_u8: sel")
        if out is None:
            out = torch.empty((Hi, Wi), dtype=torch.uint8, device=sel.device)
        if self._state_plane(out, "plane_warp_u8: out") != (Hi, Wi):
            raise SketchEditHipError("plane_warp_u8: out is a plane of sel's shape")
        by0, bx0, by1, bx1 = (int(v) for v in box)
        mm = self._warp_map(m, "plane_warp_u8")
        if self.lib.se_plane_warp_u8(self.h, self._stream(), _ptr(sel), Hi, Wi, by0, bx0, by1, bx1, mm, _ptr(out)):
            self._err("se_plane_warp_u8")
        return out

    # ---- blur, sharpen or pixelate a selection (include/sketchedit_filter.h) ----------------------------------------------
    def filter_blur_u8(self, frame, lift, lift_rect, sel, lock, box, taps, amount=-256, feather=0):
        """se_filter_blur_u8, in place on `frame` (Hi,Wi,3) uint8 on the device: the pixels of `box` = (by0, bx0, by1, bx1) that
        `sel` (an (Hi,Wi) plane, non-zero = selected) selects and `lock` (a plane or None) does not lock become the separable
        filter `taps` = [t0 .. tR] (R = 1 .. 32, t0 + 2 (t1 + .. + tR) = 4096) of the frame as `lift` holds it -- the journal slot
        window_save_u8 made of `lift_rect` = (ly0, lx0, lh, lw), a rectangle that holds the box grown by R and clipped to the
        frame -- mixed with the lifted pixel by `amount` (Q8: -256 the blur, > 0 an unsharp mask) and faded over `feather`
        pixels at the selection's rim.  No other byte changes; the frame is never read.  One launch."""
        Hi, Wi, (ly0, lx0, lh, lw), (by0, bx0, by1, bx1) = self._lift_args("filter_blur_u8", frame, lift, lift_rect, sel, lock, box)
        try:
            vals = [int(v) for v in taps]
        except (TypeError, ValueError):
            vals = []
        if not 2 <= len(vals) <= FILTER_MAX_RADIUS + 1 or any(abs(v) >= 1 << 31 for v in vals):
            raise SketchEditHipError("filter_blur_u8: taps are 2 .. %d ints [t0 .. tR]" % (FILTER_MAX_RADIUS + 1))
        tp = (ctypes.c_int * len(vals))(*vals)
        if self.lib.se_filter_blur_u8(self.h, self._stream(), _ptr(frame), Hi, Wi, _ptr(lift), ly0, lx0, lh, lw, _ptr(sel), _ptr(lock),
                                      by0, bx0, by1, bx1, tp, len(vals) - 1, int(amount), int(feather)):
            self._err("se_filter_blur_u8")

    def filter_mosaic_u8(self, frame, lift, lift_rect, sel, lock, box, cell, amount=-256, feather=0):
        """se_filter_mosaic_u8, in place on `frame`: as filter_blur_u8 with the mean of the pixel's `cell` x `cell` block (2 .. 64,
        anchored at the box's origin and clipped to the box, taken over all its lifted pixels) in place of the blur; `lift_rect`
        holds the box.  One launch."""
        Hi, Wi, (ly0, lx0, lh, lw), (by0, bx0, by1, bx1) = self._lift_args("filter_mosaic_u8", frame, lift, lift_rect, sel, lock, box)
        if self.lib.se_filter_mosaic_u8(self.h, self._stream(), _ptr(frame), Hi, Wi, _ptr(lift), ly0, lx0, lh, lw, _ptr(sel), _ptr(lock),
                                        by0, bx0, by1, bx1, int(cell), int(amount), int(feather)):
            self._err("se_filter_mosaic_u8")

    # ---- adjust a selection's tone and colour (include/sketchedit_adjust.h) ------------------------------------------------
    def adjust_u8(self, frame, lift, lift_rect, sel, lock, box, lut=None, matrix=None, amount=256, feather=0):
        """se_adjust_u8, in place on `frame` (Hi,Wi,3) uint8 on the device: the pixels of `box` = (by0, bx0, by1, bx1) that `sel`
        selects and `lock` (a plane or None) does not lock become a pointwise function of the frame as `lift` holds it -- the
        journal slot window_save_u8 made of `lift_rect` = (ly0, lx0, lh, lw), which holds the box: `lut`, 768 bytes on the device
        (a row per channel; None: the identity), THEN `matrix`, 12 ints (m[c][j] in Q12 row by row, then o[c]; None: none) --
        mixed with the lifted pixel by `amount` (Q8: 0 .. 256) and faded over `feather` pixels at the selection's rim.  No other
        byte changes; the frame is never read.  One launch."""
        Hi, Wi, (ly0, lx0, lh, lw), (by0, bx0, by1, bx1) = self._lift_args("adjust_u8", frame, lift, lift_rect, sel, lock, box)
        if lut is not None:
            _check_dev_u8(lut)
            if lut.numel() != 768:
                raise SketchEditHipError("adjust_u8: lut is 3 x 256 uint8 on the device")
        mp = None
        if matrix is not None:
            try:
                vals = [int(v) for v in matrix]
            except (TypeError, ValueError):
                vals = []
            if len(vals) != 12 or any(abs(v) >= 1 << 31 for v in vals):
                raise SketchEditHipError("adjust_u8: matrix is 12 ints, m[c][j] row by row then o[c]")
            mp = (ctypes.c_int * 12)(*vals)
        if self.lib.se_adjust_u8(self.h, self._stream(), _ptr(frame), Hi, Wi, _ptr(lift), ly0, lx0, lh, lw, _ptr(sel), _ptr(lock),
                                 by0, bx0, by1, bx1, _ptr(lut), mp, int(amount), int(feather)):
            self._err("se_adjust_u8")

    @staticmethod
    def _hist_record(t, what):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == 1024):
            raise SketchEditHipError("%s: a hist record is 4 x 256 int32 words on the device (the counts are unsigned)" % what)

    def adjust_hist_u8(self, frame, sel, box, out=None):
        """se_adjust_hist_u8: the histogram of the pixels of `box` = (by0, bx0, by1, bx1) of `frame` (Hi,Wi,3) uint8 on the device
        that `sel` selects (an (Hi,Wi) plane; None: every pixel of the box) -> a (4, 256) int32 tensor there, rows R, G, B and
        Y = (77 R + 150 G + 29 B + 128) >> 8, the counts unsigned 32-bit words.  Two launches, nothing comes down."""
        import torch
        _check_dev_u8(frame)
        if frame.dim() != 3 or frame.shape[2] != 3:
            raise SketchEditHipError("adjust_hist_u8: a frame is an (Hi,Wi,3) uint8 tensor")
        Hi, Wi = int(frame.shape[0]), int(frame.shape[1])
        if sel is not None and self._state_plane(sel, "adjust_hist_u8: sel") != (Hi, Wi):
            raise SketchEditHipError("adjust_hist_u8: sel is the frame's (Hi,Wi) plane")
        if out is None:
            out = torch.empty((4, 256), dtype=torch.int32, device=frame.device)
        self._hist_record(out, "adjust_hist_u8: out")
        need = int(self.lib.se_adjust_hist_u8_workspace_bytes(Hi, Wi))
        if need == 0:
            raise SketchEditHipError("adjust_hist_u8: bad Hi=%d Wi=%d (a frame is at least 16 x 16)" % (Hi, Wi))
        ws_t = self._workspace_bytes(need)
        by0, bx0, by1, bx1 = (int(v) for v in box)
        if self.lib.se_adjust_hist_u8(self.h, self._stream(), _ptr(frame), Hi, Wi, _ptr(sel), by0, bx0, by1, bx1, _ptr(out), _ptr(ws_t),
                                      ws_t.numel()):
            self._err("se_adjust_hist_u8")
        return out

    def adjust_lut_u8(self, hist_src, hist_ref, mode, which, clip=0, out=None):
        """se_adjust_lut_u8: one hist record of adjust_hist_u8 (and `hist_ref`, a second one, for ADJUST_MATCH only; None otherwise)
        -> the (3, 256) uint8 table on the device that adjust_u8 takes.  `mode` ADJUST_STRETCH (with `clip` 0 .. 200 per mille),
        ADJUST_EQUALIZE or ADJUST_MATCH; `which` ADJUST_PER_CHANNEL or ADJUST_LUMA.  One launch, nothing comes down."""
        import torch
        self._hist_record(hist_src, "adjust_lut_u8: hist_src")
        if hist_ref is not None:
            self._hist_record(hist_ref, "adjust_lut_u8: hist_ref")
        if out is None:
            out = torch.empty((3, 256), dtype=torch.uint8, device=hist_src.device)
        _check_dev_u8(out)
        if out.numel() != 768:
            raise SketchEditHipError("adjust_lut_u8: out is 3 x 256 uint8 on the device")
        if self.lib.se_adjust_lut_u8(self.h, self._stream(), _ptr(hist_src), _ptr(hist_ref), int(mode), int(which), int(clip), _ptr(out)):
            self._err("se_adjust_lut_u8")
        return out

    # ---- region edits ------------------------------------------------------------------------------------------
    def sketch_tiles_u8(self, sketch_u8, tile, out=None):
        """se_sketch_tiles_u8: an (Hi,Wi) uint8 plane on the device (any alignment of its base) -> (ceil(Hi / tile),
        ceil(Wi / tile), 5) int32 on the device, [count, y0, x0, y1, x1] per tile x tile square: the pixels > 0 in it and
        their tight half-open box in frame coordinates, five zeros for an empty square.  tile in {16, 32, 64}.  `out`: a
        tensor of that shape to write into (every record is written)."""
        import torch
        _check_dev_u8(sketch_u8)
        if sketch_u8.dim() != 2:
            raise SketchEditHipError("sketch_tiles_u8: a sketch is an (Hi,Wi) uint8 plane")
        Hi, Wi = sketch_u8.shape
        tile = int(tile)
        if out is None and tile > 0:
            out = torch.empty((-(-Hi // tile), -(-Wi // tile), 5), dtype=torch.int32, device=sketch_u8.device)
        if self.lib.se_sketch_tiles_u8(self.h, self._stream(), _ptr(sketch_u8), Hi, Wi, tile, _ptr(out)):
            self._err("se_sketch_tiles_u8")
        return out

    # ---- strokes as polylines -----------------------------------------------------------------------------------
    def sketch_strokes_u8(self, segs, frame_hws, origins, window_hw, ranges=None, out=None):
        """se_sketch_strokes_u8: `segs` (N,5) int32 on the device, [ax, ay, bx, by, r] in quarter pixels of the frame ->
        (B,hs,ws) uint8 on the device: the sketch of the (hs, ws) window at origins[i] = (y0, x0) of a frame of
        frame_hws[i] = (Hi, Wi), 255 where a segment of ranges[i] = (first, count) (None: all N) covers the pixel's centre by
        the integer rule of the header, 0 elsewhere.  Slice i is contiguous: what the window entries take as sketches[i].
        `out`: a contiguous uint8 tensor of B hs ws elements to write into (every byte is written)."""
        import torch
        if not (isinstance(segs, torch.Tensor) and segs.is_cuda and segs.dtype == torch.int32 and segs.is_contiguous()
                and segs.dim() == 2 and segs.shape[1] == 5):
            raise SketchEditHipError("sketch_strokes_u8: segments are an (N,5) contiguous int32 CUDA(HIP) tensor")
        hs, ws = (int(v) for v in window_hw)
        B, N = len(origins), segs.shape[0]
        if B < 1 or len(frame_hws) != B or (ranges is not None and len(ranges) != B):
            raise SketchEditHipError("sketch_strokes_u8: one frame size, one origin (and one range) per request")
        wins = (Window * B)()
        for i, ((Hi, Wi), (y0, x0)) in enumerate(zip(frame_hws, origins)):
            wins[i] = Window(None, None, int(Hi), int(Wi), int(y0), int(x0))
        flat = [int(v) for r in (ranges if ranges is not None else [(0, N)] * B) for v in r]
        if len(flat) != 2 * B:
            raise SketchEditHipError("sketch_strokes_u8: a range is (first, count)")
        rng = (ctypes.c_int * (2 * B))(*flat)
        if out is None and hs > 0 and ws > 0:
            out = torch.empty((B, hs, ws), dtype=torch.uint8, device=segs.device)
        if out is not None:
            _check_dev_u8(out)
            if out.numel() != B * hs * ws:
                raise SketchEditHipError("sketch_strokes_u8: out holds B hs ws bytes")
        if self.lib.se_sketch_strokes_u8(self.h, self._stream(), wins, B, hs, ws, _ptr(segs), N, rng, _ptr(out)):
            self._err("se_sketch_strokes_u8")
        return out

    # ---- patches as PNG ------------------------------------------------------------------------------------------
    @staticmethod
    def png_bound(hs, ws):
        """se_png_bound: the most bytes the zlib stream of an hs x ws rectangle can take; 0 for a side outside [16, 8192]
        (host only)"""
        return int(load_library().se_png_bound(int(hs), int(ws)))

    def png_encode_u8(self, frames, origins, window_hw, out=None):
        """se_png_encode_u8: the (hs, ws) rectangle at origins[i] = (y0, x0) of every frame (Hi,Wi,3) uint8 on the device -> the
        zlib stream of its PNG (include/sketchedit_png.h; serve.png_from_zlib makes the file), encoded on the device.
        -> (out (B, cap) uint8, sizes (B,) int64), both on the device: out[i, :sizes[i]] is image i's stream, and no byte
        behind it is written.  `out`: a contiguous uint8 tensor of B rows of cap >= png_bound(hs, ws) bytes to write into."""
        import torch
        hs, ws = (int(v) for v in window_hw)
        wins = self._windows(frames, origins)
        B, dev = len(frames), frames[0].device
        bound = self.png_bound(hs, ws)
        if out is None:
            out = torch.empty((B, max(bound, 1)), dtype=torch.uint8, device=dev)
        _check_dev_u8(out)
        if out.dim() != 2 or out.shape[0] != B:
            raise SketchEditHipError("png_encode_u8: `out` is a (B, cap) uint8 tensor")
        sizes = torch.empty((B,), dtype=torch.int64, device=dev)
        need = self.lib.se_png_encode_u8_workspace_bytes(self.h, B, hs, ws)
        if need == 0:
            self._err("se_png_encode_u8_workspace_bytes")
        ws_t = self._workspace_bytes(need)
        if self.lib.se_png_encode_u8(self.h, self._stream(), wins, B, hs, ws, _ptr(out), out.shape[1], _ptr(sizes), _ptr(ws_t),
                                     ws_t.numel()):
            self._err("se_png_encode_u8")
        return out, sizes

    # ---- patches as JPEG -----------------------------------------------------------------------------------------
    @staticmethod
    def jpg_bound(hs, ws):
        """se_jpg_bound: the most bytes the entropy-coded segment of an hs x ws rectangle can take; 0 for a side outside
        [16, 8192] (host only)"""
        return int(load_library().se_jpg_bound(int(hs), int(ws)))

    def jpg_encode_u8(self, frames, origins, window_hw, quality=90, out=None):
        """se_jpg_encode_u8: the (hs, ws) rectangle at origins[i] = (y0, x0) of every frame (Hi,Wi,3) uint8 on the device -> the
        entropy-coded segment of its baseline JPEG at `quality` 1 .. 100 (include/sketchedit_jpg.h; serve.jpg_from_scan makes
        the file), encoded on the device.  -> (out (B, cap) uint8, sizes (B,) int64), both on the device: out[i, :sizes[i]] is
        image i's segment, and no byte behind it is written.  `out`: a contiguous uint8 tensor of B rows of cap >=
        jpg_bound(hs, ws) bytes to write into.  It is jpg2_encode_u8 with its defaults: one encoder, se_jpg2_encode_u8 without
        flags, which is what se_jpg_encode_u8 runs."""
        return self.jpg2_encode_u8(frames, origins, window_hw, quality=quality, out=out)[:2]

    # ---- patches as JPEG, 4:2:0 and per-image Huffman tables ----------------------------------------------------------
    @staticmethod
    def jpg2_flags(subsampling="444", optimize=False):
        """("444" | "420", a bool) -> the flags of include/sketchedit_jpg2.h"""
        if not (isinstance(subsampling, str) and subsampling in ("444", "420")):
            raise SketchEditHipError("subsampling is '444' or '420' (got %r)" % (subsampling,))
        if not isinstance(optimize, bool):
            raise SketchEditHipError("optimize is a bool (got %r)" % (optimize,))
        return (SE_JPG_420 if subsampling == "420" else 0) | (SE_JPG_OPTIMIZE if optimize else 0)

    @staticmethod
    def jpg2_bound(hs, ws, flags=0):
        """se_jpg2_bound: the most bytes the segment of an hs x ws rectangle can take under `flags`; 0 for a side outside
        [16, 8192] or flags outside 0 .. 3 (host only)"""
        return int(load_library().se_jpg2_bound(int(hs), int(ws), int(flags)))

    def _jpg2_outputs(self, B, cap_min, flags, dev, out, tables, what):
        import torch
        if out is None:
            out = torch.empty((B, max(cap_min, 1)), dtype=torch.uint8, device=dev)
        _check_dev_u8(out)
        if out.dim() != 2 or out.shape[0] != B:
            raise SketchEditHipError("%s: `out` is a (B, cap) uint8 tensor" % what)
        if flags & SE_JPG_OPTIMIZE:
            if tables is None:
                tables = torch.empty((B, JPG_TABLE_RECORD_BYTES), dtype=torch.uint8, device=dev)
            _check_dev_u8(tables)
            if tuple(tables.shape) != (B, JPG_TABLE_RECORD_BYTES):
                raise SketchEditHipError("%s: `tables` is a (B, %d) uint8 tensor" % (what, JPG_TABLE_RECORD_BYTES))
        else:
            tables = None
        return out, torch.empty((B,), dtype=torch.int64, device=dev), tables

    def jpg2_encode_u8(self, frames, origins, window_hw, quality=90, subsampling="444", optimize=False, out=None, tables=None):
        """se_jpg2_encode_u8: jpg_encode_u8 with chroma at half resolution (subsampling="420") and/or four Huffman tables made
        for each image (optimize=True; include/sketchedit_jpg2.h).  -> (out (B, cap) uint8, sizes (B,) int64, tables (B, 1088)
        uint8 or None without `optimize`), all on the device; serve.jpg_from_scan makes the file from a segment and its table
        record.  `out`: B rows of cap >= jpg2_bound(hs, ws, flags) bytes to write into; `tables`: the (B, 1088) tensor to
        write the records into."""
        hs, ws = (int(v) for v in window_hw)
        flags = self.jpg2_flags(subsampling, optimize)
        wins = self._windows(frames, origins)
        B, dev = len(frames), frames[0].device
        out, sizes, tables = self._jpg2_outputs(B, self.jpg2_bound(hs, ws, flags), flags, dev, out, tables, "jpg2_encode_u8")
        need = self.lib.se_jpg2_encode_u8_workspace_bytes(self.h, B, hs, ws, flags)
        if need == 0:
            self._err("se_jpg2_encode_u8_workspace_bytes")
        ws_t = self._workspace_bytes(need)
        if self.lib.se_jpg2_encode_u8(self.h, self._stream(), wins, B, hs, ws, int(quality), flags, _ptr(out), out.shape[1], _ptr(sizes),
                                      _ptr(tables) if tables is not None else None, _ptr(ws_t), ws_t.numel()):
            self._err("se_jpg2_encode_u8")
        return out, sizes, tables

    def jpg2_code_i16(self, coef, subsampling="444", optimize=False, out=None, tables=None):
        """se_jpg2_code_i16: the stages behind the DCT on their own.  coef (B, R, nblk, 64) int16 on the device, the quantised
        coefficients in zigzag order and the stream's block order -> (out, sizes, tables) as jpg2_encode_u8.  Any int16 is
        taken: AC coefficients and DC differences are clamped to what the tables have codes for."""
        import torch
        flags = self.jpg2_flags(subsampling, optimize)
        if not (isinstance(coef, torch.Tensor) and coef.is_cuda and coef.dtype == torch.int16 and coef.is_contiguous() and coef.dim() == 4
                and coef.shape[3] == 64):
            raise SketchEditHipError("jpg2_code_i16: coef is a contiguous (B, R, nblk, 64) int16 tensor on the device")
        B, R, nblk = (int(v) for v in coef.shape[:3])
        need = self.lib.se_jpg2_code_i16_workspace_bytes(self.h, B, R, nblk, flags)
        if need == 0:
            self._err("se_jpg2_code_i16_workspace_bytes")
        bits = 1665 if flags & SE_JPG_OPTIMIZE else 1660
        out, sizes, tables = self._jpg2_outputs(B, R * (2 * ((bits * nblk + 7) // 8) + 2), flags, coef.device, out, tables, "jpg2_code_i16")
        ws_t = self._workspace_bytes(need)
        if self.lib.se_jpg2_code_i16(self.h, self._stream(), _ptr(coef), B, R, nblk, flags, _ptr(out), out.shape[1], _ptr(sizes),
                                     _ptr(tables) if tables is not None else None, _ptr(ws_t), ws_t.numel()):
            self._err("se_jpg2_code_i16")
        return out, sizes, tables

    def inference_packed(self, image, sketch, flags, out, low_latency=None):
        """Inference into ONE (B,4,H,W) buffer `out`: planes 0-2 composed, plane 3 the soft mask -- the unit the
        batch-sharded path all-gathers (sketchedit_amd/shard.py)."""
        _check_dev(image, sketch, out)
        B, _, H, W = image.shape
        assert tuple(out.shape) == (B, 4, H, W)
        ws = self.workspace(B, H, W)
        flags = (flags & 31) | self.exec_flags(B, H, W, low_latency, False) | FLAG_PACKED_OUT
        if self.lib.se_inference(self.h, self._stream(), _ptr(image), _ptr(sketch), _ptr(out), None, None, None, None,
                                 None, _ptr(ws), ws.numel(), B, H, W, flags):
            self._err("se_inference")
        return out

    # ---- measurement -----------------------------------------------------------------------------
    def profile(self, on):
        self.lib.se_profile_enable(self.h, int(on))

    def profile_report(self):
        import json
        buf = ctypes.create_string_buffer(1 << 19)      # (a full event pool: 1024 records of "launches", ~130 bytes each)
        if self.lib.se_profile_report(self.h, buf, len(buf)):
            self._err("se_profile_report")
        return json.loads(buf.value.decode())

    @contextlib.contextmanager
    def launch_forms(self):
        """Test aid: records which kernel form every launch of the body took.  Turns the profiler on (which clears earlier
        records); on exit -- also when the body raises -- turns it off again.  Yields a list that holds, after the body, one
        (form, layer) tuple per launch in launch order (se_profile_report's "launches"; DESIGN.md 3.1f names the forms)."""
        forms = []
        self.profile(True)
        try:
            yield forms
            forms.extend((r["form"], r["layer"]) for r in self.profile_report()["launches"])
        finally:
            self.profile(False)

    # ---- per-op entry points (unit tests) --------------------------------------------------------
    def gated_conv2d(self, x, w, b, stride=1, rate=1, act="elu", upsample=False, x1=None, low_latency=False, bf16=False):
        """gen_conv / gen_deconv on x, or on the virtual concat cat([x, x1]) where x1 is a (B,C1,H,W) tensor or a
        (B,C1) per-image vector (broadcast over the image, zero padded at the borders)."""
        import torch
        _check_dev(x, x1)
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        B, Cin, H, W = x.shape
        Cout, CinT, k, _ = w.shape
        Cin1 = 0 if x1 is None else x1.shape[1]
        assert CinT == Cin + Cin1
        pad = int(rate * (k - 1) / 2)
        if upsample:
            Ho, Wo = 2 * H, 2 * W
        else:
            Ho = (H + 2 * pad - rate * (k - 1) - 1) // stride + 1
            Wo = (W + 2 * pad - rate * (k - 1) - 1) // stride + 1
        raw = act is None or Cout == 3
        y = torch.empty((B, Cout if raw else Cout // 2, Ho, Wo), dtype=torch.float32, device=x.device)
        acode = {"elu": 0, "relu": 1, None: 2}[act]
        if self.lib.se_gated_conv2d_ex(self.h, self._stream(), _ptr(x), _ptr(x1), int(x1 is not None and x1.dim() == 2),
                                       w.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), _ptr(y),
                                       B, Cin, Cin1, H, W, Cout, k, stride, rate, acode, int(upsample),
                                       (FLAG_LOW_LATENCY if low_latency else 0) | (FLAG_BF16 if bf16 else 0)):
            self._err("se_gated_conv2d_ex")
        return y

    def pack_inputs(self, net, x, guide, x2=None, mask=None, mask2=None, flags=0, bf16=False):
        """se_pack_inputs: the first kernel of netM (net 'M': x = image, guide = sketch -> packed) or netG (net 'G' ->
        (coarse input, style input)), as the first conv reads them: fp32 (B,H,W,4 or 8), or with bf16 a (B,H,W,8) int16 tensor
        holding the bf16 bit patterns of one 16-byte granule per pixel."""
        import torch
        _check_dev(x, guide, x2, mask, mask2)
        B, _, H, W = x.shape
        dev = x.device

        def buf(ch):
            return torch.empty((B, H, W, 8), dtype=torch.int16, device=dev) if bf16 else \
                torch.empty((B, H, W, ch), dtype=torch.float32, device=dev)
        joint = bool(flags & FLAG_JOINT_TRAIN_INP)
        packed = buf(4 if net == "M" else 8)
        style = None if net == "M" else buf(4 if joint else 8)
        if self.lib.se_pack_inputs(self.h, self._stream(), SE_NET_M if net == "M" else SE_NET_G, _ptr(x), _ptr(x2), _ptr(mask),
                                   _ptr(mask2), _ptr(guide), _ptr(packed), _ptr(style), B, H, W, flags & 31,
                                   FLAG_BF16 if bf16 else 0):
            self._err("se_pack_inputs")
        return packed if net == "M" else (packed, style)

    def column_reduce(self, x, op, bf16=False):
        """se_column_reduce: x (B,C,H,W) -> (B,C) fp32; op 'max', 'mean' or 'rsqrt' (1 / sqrt(sum x^2 + 1e-8)).  With bf16 ->
        (fp32 result, its bf16 copy as an int16 tensor of bit patterns)."""
        import torch
        _check_dev(x)
        B, C, H, W = x.shape
        out = torch.empty((B, C), dtype=torch.float32, device=x.device)
        out16 = torch.empty((B, C), dtype=torch.int16, device=x.device) if bf16 else None
        if self.lib.se_column_reduce(self.h, self._stream(), _ptr(x), _ptr(out), _ptr(out16), B, C, H, W,
                                     {"max": 0, "mean": 1, "rsqrt": 2}[op], FLAG_BF16 if bf16 else 0):
            self._err("se_column_reduce")
        return (out, out16) if bf16 else out

    def output_conv(self, x, w, b, mode, bf16=False, no_mask_coarse=False, packed=None, **io):
        """se_output_conv: the 3x3 conv 12 -> cout with the epilogue of `mode` (0 sigmoid + threshold + lock, 1 tanh, 2 tanh +
        stage-2 input, 3 tanh + composite + uint8 outputs).  io: the tensors of se_output_conv_io by name (device tensors the
        caller allocated; absent = NULL).  packed: a (B,4,H,W) fp32 buffer -- mode 0 writes the soft mask into its plane 3, mode
        3 reads the mask there and writes the composite into planes 0-2 (`out` / `mask` / `composed` must then be absent)."""
        _check_dev(x, packed)
        w = np.ascontiguousarray(w, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        B, _, H, W = x.shape
        assert x.shape[1] == 12 and w.shape[1:] == (12, 3, 3) and b.shape == (w.shape[0],)
        ptrs = {k: (None if t is None else t.data_ptr()) for k, t in io.items()}
        if packed is not None:
            assert tuple(packed.shape) == (B, 4, H, W)
            plane3 = packed.data_ptr() + 3 * H * W * 4
            if mode == 0:
                assert "out" not in ptrs
                ptrs["out"] = plane3
            if mode == 3:
                assert "mask" not in ptrs and "composed" not in ptrs
                ptrs["mask"], ptrs["composed"] = plane3, packed.data_ptr()
        rec = OutputConvIO(**ptrs)
        if self.lib.se_output_conv(self.h, self._stream(), _ptr(x), w.ctypes.data_as(ctypes.c_void_p),
                                   b.ctypes.data_as(ctypes.c_void_p), B, H, W, w.shape[0], int(mode), ctypes.byref(rec),
                                   int(bool(no_mask_coarse)), int(packed is not None), FLAG_BF16 if bf16 else 0):
            self._err("se_output_conv")

    def quantize_u8(self, composed, mask):
        """test.py:25-27 on the device: ((composed+1)/2*255) -> uint8 (B,H,W,3) RGB, (mask*255) -> uint8 (B,H,W)."""
        import torch
        _check_dev(composed, mask)
        B, _, H, W = composed.shape
        rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=composed.device)
        m8 = torch.empty((B, H, W), dtype=torch.uint8, device=composed.device)
        if self.lib.se_quantize_u8(self.h, self._stream(), _ptr(composed), _ptr(mask), _ptr(rgb), _ptr(m8), B, H, W):
            self._err("se_quantize_u8")
        return rgb, m8

    def attention(self, x, mask_full, want_similar=False, bf16=False):
        import torch
        _check_dev(x, mask_full)
        B, C, h, w = x.shape
        assert C == 96
        hs, ws = (h - 4) // 2 + 1, (w - 4) // 2 + 1
        if want_similar:
            # se_attention_ex refuses `similar_out` where the R x R scores cannot be formed (R Rp 4 >= 2^31, R = h/2 * w/2,
            # Rp = R rounded up to 32 / 64 keys): the streaming form runs there.  Checked first: the output alone is L x L floats.
            R = (h // 2) * (w // 2)
            chunk = 64 if bf16 else 32
            if R * ((R + chunk - 1) // chunk * chunk) * 4 >= 2 ** 31:
                raise SketchEditHipError("se_attention_ex: similar_out (the %d x %d score matrix) is not available on a %dx%d "
                                         "feature map: it runs in the streaming form, which never forms it"
                                         % (hs * ws, hs * ws, h, w))
        out = torch.empty_like(x)
        sim = torch.empty((B, hs * ws, hs, ws), dtype=torch.float32, device=x.device) if want_similar else None
        if self.lib.se_attention_ex(self.h, self._stream(), _ptr(x), _ptr(mask_full), _ptr(out), _ptr(sim), B, h, w,
                                    FLAG_BF16 if bf16 else 0):
            self._err("se_attention_ex")
        return (out, sim) if want_similar else out
