"""The kernel forms of a gated convolution, one table: which call reaches which form at which sizes.

choose_form (sketchedit_amd/csrc/se_dispatch.h) chooses among some thirty kernel forms and run_gconv (se_plan.hip) launches its
choice; every launch records the form it took (Engine.launch_forms()).  FORMS holds one row per form and per just-ineligible neighbour of a
form: the call, the sizes, and the form that must run there.  tests/test_forms_host.py asks the rule for every (row, size) on
the host; tests/test_gpu_forms.py runs every (row, size) on its own -- dispatch and values against a float64 reference -- and
asserts that a whole forward launches no conv form that has no row here.

Sizes are the smallest at which a form can go wrong, not the network's: the smallest eligible size, and one with at least
two tiles on each axis and a ragged last tile (for the workgroup-tiled Winograd kernels: a tile count of B = 2 images that is
more than one workgroup and no multiple of the workgroup's 32 / 64 tiles).  Tiles: wino / wino48 / winoup 2x2 outputs, 64 per
workgroup; wino24 2x4, 32 per workgroup; rtile fp32 8x16, bf16 32x16; rtilew / rtilew2 / rconv96 16x16; rconv16 8x16 of a
polyphase sub-image; the gather-GEMM 128 output pixels (n96: 192), 64 in its small-grid shape.
"""
import collections

import numpy as np
import torch

from sketchedit_amd import synth

BATCH = 2
TOL_OP = 1e-4            # the project's per-op bound in fp32 (tests/test_gpu_parity.py)
TOL_BF16_DECONV = 2e-2   # sub-pixel bf16 deconv: pre-summed weights rounded once (tests/test_gpu_bf16.py)

# a launch is a conv launch when its form starts with one of these (layout converters, packing, reductions, attention do not)
CONV_PREFIXES = ("gconv_", "wino", "rtile", "rconv", "vecbias", "small_conv")

Row = collections.namedtuple("Row", "form cin cout k stride rate up src2 mode switches shapes pre act note")


def row(form, cin, cout, shapes, k=3, stride=1, rate=1, up=False, src2=None, mode="default", switches=None, pre=(), act="elu", note=""):
    """form: the form that must run.  src2: None, 'tensor' or 'vector' (cin counts BOTH sources: 96 + 96).  mode: 'default',
    'lowlat' or 'bf16'.  switches: developer switches set for the call.  pre: forms launched in front of it ('vecbias')."""
    return Row(form, cin, cout, k, stride, rate, up, src2, mode, dict(switches or {}), list(shapes), tuple(pre), act, note)


FORMS = [
    # ---- fp32, default mode: 96 -> 192 3x3 stride 1 -------------------------------------------------------------------
    # wino24: h % 2d == 0, w % 4d == 0.  10x20: 50 tiles = 2 workgroups, the second ragged; 12x24 at d = 2 and d = 3: 72 tiles
    row("wino24", 96, 192, [(2, 4), (10, 20)]),
    row("wino24", 96, 192, [(4, 8), (12, 24)], rate=2),
    row("wino24", 96, 192, [(6, 12), (12, 24)], rate=3, act="relu"),
    # neighbours: w % 4d != 0 -> wino (70, 60, 108 tiles: more than one 64-tile workgroup, ragged); odd h or w -> gather-GEMM
    row("wino", 96, 192, [(2, 2), (10, 14)], note="wino24 with w % 4 != 0"),
    row("wino", 96, 192, [(4, 4), (12, 20)], rate=2, note="wino24 with w % 4d != 0"),
    row("wino", 96, 192, [(6, 6), (12, 18)], rate=3, note="wino24 with w % 4d != 0"),
    row("wino", 96, 192, [(4, 8), (10, 20)], switches={"SE_WINOGRAD_F43": 0}, act="relu"),
    row("gconv_n192", 96, 192, [(3, 4), (9, 20), (10, 19)], note="wino24 / wino with odd h or w"),
    row("gconv_n192", 96, 192, [(10, 20), (12, 22)], rate=2, note="wino at d = 2 with h % 2d != 0 / w % 2d != 0"),
    row("gconv_n192", 96, 192, [(10, 20)], switches={"SE_WINOGRAD": 0}),
    # two sources (conv11 / allconv11): a tensor, or the pooled vector folded into a bias table
    row("wino24_2src", 192, 192, [(2, 4), (10, 20)], src2="tensor"),
    row("wino_2src", 192, 192, [(2, 2), (10, 14)], src2="tensor", note="wino24_2src with w % 4 != 0"),
    row("gconv_n192_2src", 192, 192, [(3, 4), (9, 20)], src2="tensor", note="wino24_2src with odd h"),
    row("wino24", 192, 192, [(2, 4), (10, 20)], src2="vector", pre=("vecbias",)),
    row("wino", 192, 192, [(2, 2), (10, 14)], src2="vector", pre=("vecbias",), note="folded wino24 with w % 4 != 0"),
    row("wino_2src", 192, 192, [(2, 4), (10, 20)], src2="vector", switches={"SE_VECBIAS": 0}, note="folded vector switched off"),
    row("gconv_n192_2src", 192, 192, [(9, 20)], src2="vector", note="folded vector with odd h"),
    # ---- fp32: the other Winograd layers -------------------------------------------------------------------------------
    row("wino24_c48", 48, 192, [(2, 4), (10, 20)]),
    row("wino24_c48", 48, 192, [(12, 24)], rate=2),
    row("wino24_c48", 48, 192, [(12, 24)], rate=3),
    row("gconv_n192", 48, 192, [(10, 18), (9, 20)], note="wino24_c48 with w % 4 != 0 / odd h"),
    row("wino48", 48, 96, [(2, 2), (10, 14)]),
    row("wino48", 48, 96, [(12, 20)], rate=2),
    row("wino48", 48, 96, [(12, 18)], rate=3, act="relu"),
    row("gconv_n96", 48, 96, [(9, 14), (10, 13)], note="wino48 with odd h / w"),
    row("wino48_c24", 24, 96, [(2, 2), (10, 14)]),
    row("wino48_c24", 24, 96, [(12, 20)], rate=2),
    row("wino48_c24", 24, 96, [(12, 18)], rate=3),
    row("gconv_n96", 24, 96, [(9, 14), (10, 13)], note="wino48_c24 with odd h / w"),
    row("gconv_n96", 24, 96, [(10, 14)], switches={"SE_WINOGRAD48": 0}),
    row("winoup", 96, 96, [(2, 2), (10, 14)], up=True),
    row("gconv_n96_up2", 96, 96, [(9, 14), (10, 13)], up=True, note="winoup with odd h / w"),
    row("winoup48", 48, 48, [(2, 2), (10, 14)], up=True),
    row("rtile_up2", 48, 48, [(3, 2), (9, 18), (10, 17)], up=True, note="winoup48 with odd h / w"),
    row("gconv_n48_up2", 48, 48, [(9, 18)], up=True, switches={"SE_RTILE": 0}),
    # ---- fp32: raw-tile forms of the narrow layers ----------------------------------------------------------------------
    row("rtilew2", 24, 24, [(2, 2), (18, 34)]),
    row("rtilew", 24, 24, [(3, 2), (17, 34)], note="rtilew2 with odd h"),
    row("rtile", 24, 24, [(2, 3), (9, 17), (18, 33)], note="rtilew2 / rtilew with odd w"),
    row("rtilew", 24, 24, [(18, 34)], switches={"SE_RTILE_WX": 1}),
    row("rtile", 24, 24, [(18, 34)], switches={"SE_RTILE_WX": 0}),
    row("gconv_n24", 24, 24, [(3, 3), (9, 17)], switches={"SE_RTILE": 0}),
    row("gconv_n24", 24, 24, [(9, 17)], rate=2, note="raw tiles need rate 1"),
    row("rtile_dense5w", 5, 48, [(5, 2), (9, 18)], k=5),
    row("rtile_dense5w", 3, 48, [(9, 18)], k=5),
    row("rtile_dense5w", 4, 48, [(9, 18)], k=5),
    row("rtile_dense5", 5, 48, [(2, 3), (9, 17)], k=5, note="rtile_dense5w with odd w"),
    row("rtile_dense5", 3, 48, [(9, 17)], k=5, note="rtile_dense5w with odd w"),
    row("rtile_dense5", 4, 48, [(9, 18)], k=5, switches={"SE_RTILE_D5W": 0}),
    row("rtile", 5, 48, [(9, 17)], k=5, switches={"SE_RTILE_DENSE": 0}),
    # ---- fp32: strided layers (gather-GEMM only) -----------------------------------------------------------------------
    row("gconv_n192", 48, 192, [(2, 2), (22, 18)], stride=2),
    row("gconv_n96", 24, 96, [(2, 2), (22, 18), (40, 66)], stride=2),
    row("gconv_n96", 48, 96, [(22, 18)], stride=2),
    row("gconv_n48", 24, 48, [(2, 2), (22, 18)], stride=2),
    # the raw output convs
    row("small_conv", 12, 3, [(2, 2), (9, 17)], act=None),
    row("small_conv", 12, 1, [(9, 17)], act=None),
    # ---- fp32, low-latency mode at the default thresholds: the small-grid gather-GEMM (64-pixel tiles) ------------------
    row("gconv_n192_small", 96, 192, [(2, 4), (10, 20)], mode="lowlat"),
    row("gconv_n192_small", 96, 192, [(12, 24)], rate=2, mode="lowlat"),
    row("gconv_n192_small_2src", 192, 192, [(10, 20)], src2="tensor", mode="lowlat"),
    row("gconv_n192_small_2src", 192, 192, [(10, 20)], src2="vector", mode="lowlat"),
    row("gconv_n192_small", 48, 192, [(10, 20)], mode="lowlat"),
    row("gconv_n192_small", 48, 192, [(22, 18)], stride=2, mode="lowlat"),
    row("gconv_n96_small", 48, 96, [(10, 14)], mode="lowlat"),
    row("gconv_n96_small", 24, 96, [(10, 14)], mode="lowlat"),
    row("gconv_n96_small", 24, 96, [(22, 18)], stride=2, mode="lowlat"),
    row("gconv_n96_small_up2", 96, 96, [(10, 14)], up=True, mode="lowlat"),
    row("gconv_n48_small_up2", 48, 48, [(10, 14), (9, 17)], up=True, mode="lowlat"),
    row("gconv_n48_small", 24, 48, [(22, 18)], stride=2, mode="lowlat"),
    row("gconv_n48_small", 5, 48, [(9, 18)], k=5, mode="lowlat"),
    row("gconv_n24_small", 24, 24, [(2, 2), (18, 34)], mode="lowlat"),
    # ---- bf16 mode: 96 -> 192 3x3 stride 1 -----------------------------------------------------------------------------
    # rconv16: h / d >= 12 and w / d >= 12 (8x16 tiles of a polyphase sub-image; 22x36: 3 x 3 tiles, ragged both ways)
    row("rconv16", 96, 192, [(12, 12), (22, 36)], mode="bf16"),
    row("rconv16", 96, 192, [(24, 24), (26, 36)], rate=2, mode="bf16"),
    row("rconv16", 96, 192, [(36, 39)], rate=3, mode="bf16", act="relu"),
    row("gconv_n192_bf16", 96, 192, [(11, 12), (12, 11)], mode="bf16", note="rconv16 with h / d == 11 or w / d == 11"),
    row("gconv_n192_bf16", 96, 192, [(22, 24)], rate=2, mode="bf16", note="rconv16 with h / d == 11"),
    row("gconv_n192_bf16", 96, 192, [(25, 24)], rate=2, mode="bf16", note="rconv16 with h % d != 0"),
    row("gconv_n192_bf16", 96, 192, [(22, 36)], mode="bf16", switches={"SE_RCONV16": 0}),
    # rconv16_dual: d even, w / d == 8, 4 <= h / d <= 8
    row("rconv16_dual", 96, 192, [(8, 16), (16, 16), (10, 16)], rate=2, mode="bf16"),
    row("rconv16_dual", 96, 192, [(24, 48)], rate=6, mode="bf16"),
    row("gconv_n192_bf16", 96, 192, [(6, 16), (18, 16), (8, 18)], rate=2, mode="bf16", note="rconv16_dual with h / d == 3, 9; w / d == 9"),
    row("gconv_n192_bf16", 96, 192, [(12, 24)], rate=3, mode="bf16", note="rconv16_dual needs an even d"),
    row("gconv_n192_bf16", 96, 192, [(16, 16)], rate=2, mode="bf16", switches={"SE_RCONV16_DUAL": 0}),
    # the folded vector source: vecbias (vector rounded to bf16) + rconv16 on the first source; h, w >= 12
    row("rconv16", 192, 192, [(12, 12), (22, 36)], src2="vector", mode="bf16", pre=("vecbias",)),
    row("gconv_n192_2src_bf16", 192, 192, [(11, 12), (12, 11)], src2="vector", mode="bf16", note="folded rconv16 with h == 11 / w == 11"),
    row("gconv_n192_2src_bf16", 192, 192, [(14, 18)], src2="vector", mode="bf16", switches={"SE_VECBIAS": 0}),
    row("gconv_n192_2src_bf16", 192, 192, [(14, 18)], src2="tensor", mode="bf16"),
    # ---- bf16: the 96-row layers (rconv96, 16x16 tiles; h, w >= 12) ----------------------------------------------------
    row("rconv96", 48, 96, [(12, 12), (22, 36)], mode="bf16"),
    row("rconv96_c24", 24, 96, [(12, 12), (22, 36)], mode="bf16"),
    row("rconv96_s2", 24, 96, [(12, 12), (40, 66), (23, 35)], stride=2, mode="bf16"),
    row("rconv96_up", 96, 96, [(12, 12), (22, 36)], up=True, mode="bf16"),
    row("gconv_n96_bf16", 48, 96, [(11, 12), (12, 11)], mode="bf16", note="rconv96 with h == 11 / w == 11"),
    row("gconv_n96_bf16", 24, 96, [(11, 12)], mode="bf16", note="rconv96_c24 with h == 11"),
    row("gconv_n96_bf16", 24, 96, [(11, 12), (12, 11)], stride=2, mode="bf16", note="rconv96_s2 with h == 11 / w == 11"),
    row("gconv_n96_up2_bf16", 96, 96, [(11, 12)], up=True, mode="bf16", note="rconv96_up with h == 11"),
    row("gconv_n96_bf16", 48, 96, [(22, 36)], mode="bf16", switches={"SE_RCONV96": 0}),
    row("gconv_n96_bf16", 48, 96, [(22, 36)], rate=2, mode="bf16", note="rconv96 needs rate 1"),
    row("gconv_n96_bf16", 48, 96, [(22, 18)], stride=2, mode="bf16"),
    # ---- bf16: narrow layers (rtile, 32x16 tiles) and the rest ------------------------------------------------------------
    row("rtile_bf16", 24, 24, [(2, 2), (34, 18), (33, 17)], mode="bf16"),
    row("rtile_bf16", 5, 48, [(34, 18)], k=5, mode="bf16"),
    row("rtile_bf16_up2", 48, 48, [(2, 2), (34, 18), (33, 17)], up=True, mode="bf16"),
    row("rtile_bf16_d4", 3, 48, [(2, 2), (34, 18), (33, 17)], k=5, mode="bf16"),
    row("rtile_bf16_d4", 4, 48, [(33, 17)], k=5, mode="bf16"),
    row("rtile_bf16", 4, 48, [(33, 17)], k=5, mode="bf16", switches={"SE_RTILE_DENSE": 0}),
    row("gconv_n24_bf16", 24, 24, [(9, 17)], mode="bf16", switches={"SE_RTILE": 0}),
    row("gconv_n48_up2_bf16", 48, 48, [(9, 17)], up=True, mode="bf16", switches={"SE_RTILE": 0}),
    row("gconv_n192_bf16", 48, 192, [(22, 18)], stride=2, mode="bf16"),
    row("gconv_n192_bf16", 48, 192, [(22, 36)], mode="bf16"),
    row("gconv_n48_bf16", 24, 48, [(22, 18)], stride=2, mode="bf16"),
    row("small_conv", 12, 3, [(9, 17)], act=None, mode="bf16"),
]

# the forms of the low-latency and bf16 modes together (the whole-forward test runs bf16 forwards in low-latency mode too)
FORMS += [
    row("gconv_n192_small_bf16", 96, 192, [(12, 12), (22, 36)], mode="bf16-lowlat", note="rconv16 in low-latency mode"),
    row("gconv_n192_small_bf16", 96, 192, [(16, 16)], rate=2, mode="bf16-lowlat", note="rconv16_dual in low-latency mode"),
    row("gconv_n192_small_2src_bf16", 192, 192, [(14, 18)], src2="vector", mode="bf16-lowlat", note="folded rconv16 in low-latency mode"),
    row("gconv_n192_small_2src_bf16", 192, 192, [(14, 18)], src2="tensor", mode="bf16-lowlat"),
    row("gconv_n192_small_bf16", 48, 192, [(22, 18)], stride=2, mode="bf16-lowlat"),
    row("gconv_n96_small_bf16", 48, 96, [(22, 36)], mode="bf16-lowlat", note="rconv96 in low-latency mode"),
    row("gconv_n96_small_bf16", 24, 96, [(40, 66)], stride=2, mode="bf16-lowlat", note="rconv96_s2 in low-latency mode"),
    row("gconv_n96_small_up2_bf16", 96, 96, [(22, 36)], up=True, mode="bf16-lowlat", note="rconv96_up in low-latency mode"),
    row("gconv_n48_small_up2_bf16", 48, 48, [(33, 17)], up=True, mode="bf16-lowlat"),
    row("gconv_n48_small_bf16", 24, 48, [(22, 18)], stride=2, mode="bf16-lowlat"),
    row("gconv_n48_small_bf16", 3, 48, [(33, 17)], k=5, mode="bf16-lowlat"),
    row("gconv_n24_small_bf16", 24, 24, [(33, 17)], mode="bf16-lowlat"),
]

# Low-latency mode: the Winograd / raw-tile kernels run from a threshold of workgroups (tiles) PER IMAGE on.  (row, switch, count
# of the row's LAST shape): with the switch at `count` the row's form runs, with it at count + 1 the small-grid form `below`.
LowLat = collections.namedtuple("LowLat", "row switch count below")
LL_THRESHOLDS = [
    LowLat(row("wino24", 96, 192, [(16, 20)]), "SE_LL_WINO_MIN_WG", 2, "gconv_n192_small"),                 # ceil(8 * 10 / 64)
    LowLat(row("wino", 96, 192, [(16, 18)]), "SE_LL_WINO_MIN_WG", 2, "gconv_n192_small"),                   # ceil(8 * 9 / 64)
    LowLat(row("wino24", 192, 192, [(16, 20)], src2="vector", pre=("vecbias",)), "SE_LL_WINO_MIN_WG", 2, "gconv_n192_small_2src"),
    LowLat(row("wino24_2src", 192, 192, [(16, 20)], src2="tensor"), "SE_LL_WINO_MIN_WG", 2, "gconv_n192_small_2src"),
    LowLat(row("wino24_c48", 48, 192, [(16, 20)]), "SE_LL_WINO_MIN_WG", 2, "gconv_n192_small"),             # ceil(8 * 5 / 32)
    LowLat(row("wino48", 48, 96, [(16, 18)]), "SE_LL_WINO48_MIN_WG", 2, "gconv_n96_small"),
    LowLat(row("wino48_c24", 24, 96, [(16, 18)]), "SE_LL_WINO48_MIN_WG", 2, "gconv_n96_small"),
    LowLat(row("winoup", 96, 96, [(16, 18)], up=True), "SE_LL_WINO48_MIN_WG", 8, "gconv_n96_small_up2"),    # 4 classes x 2
    LowLat(row("winoup48", 48, 48, [(16, 18)], up=True), "SE_LL_WINO48_MIN_WG", 8, "gconv_n48_small_up2"),
    LowLat(row("rtilew2", 24, 24, [(18, 34)]), "SE_RTILE_LL_MIN", 9, "gconv_n24_small"),                    # 8x16 tiles: 3 x 3
    LowLat(row("rtile_dense5w", 5, 48, [(18, 34)], k=5), "SE_RTILE_LL_MIN", 9, "gconv_n48_small"),
    LowLat(row("rtile_up2", 48, 48, [(9, 17)], up=True), "SE_RTILE_LL_MIN", 16, "gconv_n48_small_up2"),     # 2 x 2 tiles x 4 classes
    LowLat(row("rtile_bf16", 24, 24, [(34, 18)], mode="bf16"), "SE_RTILE_LL_MIN", 4, "gconv_n24_small_bf16"),   # 32x16 tiles: 2 x 2
]


# The arithmetic family of a form: which Winograd-type transforms lie between the operands and the sum (se_pack.hip and the
# kernels' header comments).  Everything not named here multiplies the operands as they are ('direct'): the
# gather-GEMM forms, rtile / rtile_up2 / rtile_dense5 / rtile_bf16*, rconv16*, rconv96*, small_conv.
FAMILY = {
    "wino": "f23xf23", "wino_2src": "f23xf23", "wino48": "f23xf23", "wino48_c24": "f23xf23", "rtilew2": "f23xf23",
    "wino24": "f23xf43", "wino24_2src": "f23xf43", "wino24_c48": "f23xf43",
    "rtilew": "f23x",
    "rtile_dense5w": "f25x",
    "winoup": "subpixel", "winoup48": "subpixel",
}


def family(form):
    """'direct', 'f23xf23' (F(2,3) x F(2,3)), 'f23xf43' (F(2,3) x F(4,3)), 'f23x' (F(2,3) along x), 'f25x' (F(2,5) along x) or
    'subpixel' (F(2x2,2x2) on the sub-pixel classes of gen_deconv)."""
    if form in FAMILY:
        return FAMILY[form]
    assert form.startswith(("gconv_", "rtile", "rconv", "small_conv", "vecbias")) and not form.startswith(("rtilew", "rtile_dense5w")), form
    return "direct"


def conv_launches(launches):
    """The conv launches among (form, layer) records, as a list of forms."""
    return [f for f, _ in launches if f.startswith(CONV_PREFIXES)]


def conv_as(eng, expected, *args, **kw):
    """eng.gated_conv2d(*args, **kw), asserting that its conv launches are exactly `expected` (one form name, or a list)."""
    with eng.launch_forms() as launches:
        y = eng.gated_conv2d(*args, **kw)
    want = [expected] if isinstance(expected, str) else list(expected)
    assert conv_launches(launches) == want, launches
    return y


def known_forms():
    s = {r.form for r in FORMS} | {t.row.form for t in LL_THRESHOLDS} | {t.below for t in LL_THRESHOLDS}
    for r in FORMS:
        s.update(r.pre)
    return s


def row_id(r, shape=None):
    s = "%s-%s-%dto%d-k%d-s%d-d%d%s%s" % (r.form, r.mode, r.cin, r.cout, r.k, r.stride, r.rate, "-up" if r.up else "",
                                          "-" + r.src2 if r.src2 else "")
    for k, v in sorted(r.switches.items()):
        s += "-%s=%s" % (k[3:], v)
    if shape is not None:
        s += "-%dx%d" % shape
    return s


def cases():
    """Every (row, shape) of FORMS."""
    return [(r, s) for r in FORMS for s in r.shapes]


def make_inputs(r, shape, B=BATCH):
    """-> x (B,C0,H,W), x1 (None, (B,96,H,W) or (B,96)), w, b as float32 arrays; different images within the batch."""
    H, W = shape
    key = "%s|%dx%d|%d" % (row_id(r), H, W, B)
    c0 = r.cin - (96 if r.src2 else 0)
    a = 1.5 / np.sqrt(r.cin * r.k * r.k)
    w = synth.uniform(71, "forms.w" + key, (r.cout, r.cin, r.k, r.k), -a, a)
    b = synth.uniform(71, "forms.b" + key, (r.cout,), -0.3, 0.3)
    x = synth.uniform(71, "forms.x" + key, (B, c0, H, W), -1, 1)
    x1 = None
    if r.src2 == "tensor":
        x1 = synth.uniform(71, "forms.y" + key, (B, 96, H, W), -1, 1)
    elif r.src2 == "vector":
        x1 = synth.uniform(71, "forms.v" + key, (B, 96), -1, 1)
    return x, x1, w, b


def reference(r, x, x1, w, b):
    """float64 reference of the same operation on the CPU: conv2d in double (on the nearest-x2 input for `up`, the second
    source concatenated explicitly -- a vector broadcast over the image, zero padded like a tensor), then ELU|ReLU(features) *
    sigmoid(gates); the raw conv for act None.  bf16 mode: inputs and weights rounded to bf16 first, the result rounded to
    bf16 (what the layer stores)."""
    bf = r.mode.startswith("bf16")
    rnd = (lambda a: torch.from_numpy(a).to(torch.bfloat16).double()) if bf else (lambda a: torch.from_numpy(a).double())
    tx = rnd(x)
    if x1 is not None:
        t1 = rnd(x1)
        if t1.dim() == 2:
            t1 = t1[:, :, None, None].expand(-1, -1, tx.shape[2], tx.shape[3])
        tx = torch.cat([tx, t1], 1)
    if r.up:
        tx = tx.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    pad = r.rate * (r.k - 1) // 2
    y = torch.nn.functional.conv2d(tx, rnd(w), torch.from_numpy(b).double(), stride=r.stride, padding=pad, dilation=r.rate)
    if r.act is not None:
        f, g = y[:, : r.cout // 2], y[:, r.cout // 2:]
        f = torch.nn.functional.elu(f) if r.act == "elu" else torch.relu(f)
        y = f * torch.sigmoid(g)
        if bf:
            y = y.to(torch.bfloat16).double()
    return y


def predict(r, shape, B=BATCH, mode=None):
    """The conv launches of row r's call as the library's rule answers on the host (se_debug_gconv_form: choose_form, the function
    run_gconv launches by) -- no device."""
    from sketchedit_amd import _lib
    mode = r.mode if mode is None else mode
    c1 = 96 if r.src2 else 0
    return _lib.gconv_form(r.cin - c1, r.cout, shape[0], shape[1], k=r.k, stride=r.stride, rate=r.rate, act=r.act, upsample=r.up, cin1=c1,
                           x1_is_vector=r.src2 == "vector", B=B, low_latency="lowlat" in mode, bf16=mode.startswith("bf16"))


def dump_rows():
    """Every (row, shape) of FORMS as a line of tools/dispatch_host_check.hip's input: the arguments of se_debug_gconv_form, the
    expected launches, the row's switches."""
    for r, (H, W) in cases():
        c1 = 96 if r.src2 else 0
        flags = (32 if "lowlat" in r.mode else 0) | (256 if r.mode.startswith("bf16") else 0)
        print(r.cin - c1, c1, int(r.src2 == "vector"), r.cout, r.k, r.stride, r.rate, {"elu": 0, "relu": 1, None: 2}[r.act], int(r.up), BATCH, H, W,
              flags, 0, ",".join(list(r.pre) + [r.form]), *["%s=%d" % kv for kv in sorted(r.switches.items())])


def run(eng, r, x, x1, w, b):
    """The call of row r on the GPU -> (output tensor, the (form, layer) records of its launches)."""
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()      # noqa: E731
    with eng.launch_forms() as launches:
        y = eng.gated_conv2d(cu(x), w, b, stride=r.stride, rate=r.rate, act=r.act, upsample=r.up, x1=cu(x1),
                             low_latency="lowlat" in r.mode, bf16=r.mode.startswith("bf16"))
    return y, launches
