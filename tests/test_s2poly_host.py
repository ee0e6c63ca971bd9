"""The polyphase F(2,2) form of the 48-channel stride-2 gated convs ("s2poly48", sketchedit_amd/csrc/se_s2poly.h)
on the host: the rule that chooses it (choose_form through se_debug_gconv_form), its position tables and its weight packer
(the derived entries SE_S2POLY_TABLE / SE_S2POLY_PACK of se_debug_get_option) against a float64 model.  No device is needed:
all three are host arithmetic of the library.

The model.  A 3-tap stride-2 conv with padding 1 gives, per output pair o0 = out[2t], o1 = out[2t+1] over the patch
i_m = in[4t+m] (m = -1..3, patch index m + 1), five products:
    i0 w1 -> o0;  i2 w1 -> o1;  (i-1 - i1) w0 -> o0;  i1 (w0 + w2) -> o0 and o1;  (i1 - i3) w2 -> -o1
and the two-dimensional form is the outer product: 25 products per 2x2 output tile instead of 36.
"""
import numpy as np
import pytest

from sketchedit_amd import _lib, synth
import forms_util as FU

FORM = "s2poly48"
SIZES = [(8, 8), (12, 20), (64, 64)]
OLD = {96: "gconv_n96", 192: "gconv_n192"}


def _ask(cin, cout, H, W, B=1, **kw):
    kw.setdefault("stride", 2)
    return _lib.gconv_form(cin, cout, H, W, B=B, **kw)


# ---- 1: the rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout", [96, 192])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_rule_takes_the_form_at_multiples_of_four(cout, size):
    for B in (1, 2, 3):
        assert _ask(48, cout, *size, B=B) == [FORM], B
        assert _ask(48, cout, *size, B=B, act="relu") == [FORM], B
        assert _ask(48, cout, *size, B=B, net=_lib.SE_NET_M) == [FORM], B


@pytest.mark.parametrize("cout", [96, 192])
def test_rule_keeps_the_gather_form_elsewhere(cout, seopt):
    old = OLD[cout]
    for H, W in [(10, 8), (8, 10), (6, 6), (22, 18), (9, 8), (8, 7), (2, 2)]:      # either side no multiple of 4
        assert _ask(48, cout, H, W) == [old], (H, W)
    for size in SIZES:
        assert _ask(48, cout, *size, low_latency=True) == [old + "_small"]
        assert _ask(48, cout, *size, bf16=True) == [old + "_bf16"]
        assert _ask(48, cout, *size, rate=2) == [old]
    # 24-channel layers stay where they are, whatever the size
    assert _ask(24, 96, 64, 64) == ["gconv_n96"] and _ask(24, 48, 64, 64) == ["gconv_n48"]
    # stride 1 is not this form's
    assert _ask(48, 96, 8, 8, stride=1) == ["wino48"]
    # the byte range: B H W 192 < 2^31
    assert _ask(48, cout, 1024, 1024, B=10) == [FORM] and _ask(48, cout, 1024, 1024, B=11) == [old]
    # the switch: 0 off, 2 netG only
    seopt.set("SE_S2_POLY", 0)
    for size in SIZES:
        assert _ask(48, cout, *size) == [old]
    seopt.set("SE_S2_POLY", 2)
    assert _ask(48, cout, 8, 8, net=_lib.SE_NET_G) == [FORM] and _ask(48, cout, 8, 8, net=_lib.SE_NET_M) == [old]


def test_switch_default_is_on():
    assert _lib.get_option("SE_S2_POLY") in (0, 1, 2)      # (the built-in default, 1, is asserted below in a scrubbed child)
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("SE_")}
    out = subprocess.run([sys.executable, "-c", "from sketchedit_amd import _lib; print(_lib.get_option('SE_S2_POLY'))"], cwd=root, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.split() == ["1"], out


STRIDED = [(r, s) for r, s in FU.cases() if r.stride == 2]


def test_no_strided_row_of_the_table_is_at_a_multiple_of_four():
    """The form table's strided rows keep their answers because none has both sides divisible by 4 -- verified, not assumed."""
    assert len(STRIDED) >= 15
    assert not [(FU.row_id(r, s)) for r, s in STRIDED if s[0] % 4 == 0 and s[1] % 4 == 0 and r.cin == 48]


@pytest.mark.parametrize("case", STRIDED, ids=[FU.row_id(r, s) for r, s in STRIDED])
def test_strided_rows_of_the_table_are_unchanged(case, seopt):
    r, shape = case
    for name, v in r.switches.items():
        seopt.set(name, v)
    for B in (1, 2, 3):
        assert FU.predict(r, shape, B=B) == list(r.pre) + [r.form]


# ---- 2: the position tables ---------------------------------------------------------------------------------------------------
def _tables():
    t = _lib.s2poly_tables()
    assert t.shape == (5, 7)
    return t


def test_tables_are_the_documented_ones():
    want = [[1, -1, 0, 1, 0, 1, 0], [3, -1, 0, 1, 0, 0, 1], [0, 2, 1, 0, 0, 1, 0], [2, -1, 1, 0, 1, 1, 1], [2, 4, 0, 0, 1, 0, -1]]
    assert _tables().tolist() == want
    t = _tables()
    nsrc = 1 + (t[:, 1] >= 0)
    assert int(nsrc.sum()) ** 2 == 49 and sorted(np.outer(nsrc, nsrc).ravel().tolist()).count(4) == 4


def _direct_tile(patch, g):
    """The 2x2 outputs of a 3x3 stride-2 conv whose 5x5 source patch (rows / columns 4t-1 .. 4t+3) is `patch`, in float64."""
    out = np.zeros((2, 2))
    for a in range(2):
        for b in range(2):
            out[a, b] = (patch[2 * a:2 * a + 3, 2 * b:2 * b + 3] * g).sum()
    return out


def _folded_tile(t, patch, g):
    """The same from the 25 products of the tables: source sums, transformed weights, fold."""
    out = np.zeros((2, 2))
    n = 0
    for py in range(5):
        for px in range(5):
            ya, yb, xa, xb = t[py, 0], t[py, 1], t[px, 0], t[px, 1]
            src = patch[ya, xa]
            if xb >= 0:
                src = src - patch[ya, xb]
            if yb >= 0:
                src = src - patch[yb, xa] + (patch[yb, xb] if xb >= 0 else 0.0)
            u = (np.outer(t[py, 2:5], t[px, 2:5]) * g).sum()
            for a in range(2):
                for b in range(2):
                    out[a, b] += t[py, 5 + a] * t[px, 5 + b] * (src * u)
            n += 1
    assert n == 25
    return out


def test_tables_fold_to_the_direct_outputs():
    t = _tables().astype(np.int64)
    rng = np.random.RandomState(29)
    worst = 0.0
    for _ in range(200):
        g, patch = rng.uniform(-1, 1, (3, 3)), rng.uniform(-1, 1, (5, 5))
        worst = max(worst, float(np.abs(_folded_tile(t, patch, g) - _direct_tile(patch, g)).max()))
    # border tiles: the padding row / column reads as zero in both
    for _ in range(20):
        g, patch = rng.uniform(-1, 1, (3, 3)), rng.uniform(-1, 1, (5, 5))
        patch[0, :] = 0
        patch[:, 0] = 0
        worst = max(worst, float(np.abs(_folded_tile(t, patch, g) - _direct_tile(patch, g)).max()))
    assert worst <= 1e-12, worst


# ---- 3: the packer ----------------------------------------------------------------------------------------------------------------
def _mixed_channel(n, G):
    f = n // 16 * 8 + n % 8
    return f if n % 16 < 8 else G + f


@pytest.mark.parametrize("cout", [96, 192])
def test_packer_matches_the_model(cout):
    """The library's packer on the probe layer (every weight a multiple of 1/1024: no two of the 25 transformed weights of a
    kernel coincide by accident of zeros), element by element against the model in float64, rounded once."""
    t = _tables().astype(np.int64)
    w, b = _lib.s2poly_probe_layer(cout)
    assert len(np.unique(w)) > 2000 and float(np.abs(w).max()) <= 1026 / 1024
    img, bias = _lib.s2poly_probe_pack(cout)
    assert img.shape == (cout // 96, 38, 96, 32) and bias.shape == (cout,)
    want = np.zeros(img.shape, np.float64)
    seen = np.zeros(img.shape, bool)
    rows = np.array([_mixed_channel(n, cout // 2) for n in range(cout)])
    assert sorted(rows.tolist()) == list(range(cout))
    assert np.array_equal(bias, b[rows])
    w64 = w.astype(np.float64)
    for pos in range(25):
        py, px = divmod(pos, 5)
        u = np.einsum("oiyx,y,x->oi", w64, t[py, 2:5].astype(np.float64), t[px, 2:5].astype(np.float64))      # (cout, 48)
        for ic in range(48):
            u6 = (pos & 1) * 3 + ic // 16
            it, kin = (pos >> 1) * 3 + u6 // 2, (u6 % 2) * 16 + ic % 16
            for n in range(cout):
                r = n % 96
                k = ((kin // 4) ^ ((r >> 1) & 7)) * 4 + kin % 4
                want[n // 96, it, r, k] = u[rows[n], ic]
                seen[n // 96, it, r, k] = True
    # every k of every chunk is written once but the k-half behind position 24, which stays zero
    assert int((~seen).sum()) == (cout // 96) * 96 * 16 and not img[~seen].any()
    logical_half1 = np.zeros(img.shape, bool)
    for r in range(96):
        for s in range(4, 8):
            k0 = (s ^ ((r >> 1) & 7)) * 4
            logical_half1[:, 37, r, k0:k0 + 4] = True
    assert np.array_equal(~seen, logical_half1)
    # formed in float64 and rounded once
    assert np.array_equal(img, want.astype(np.float32))


def test_packer_refuses_other_widths():
    v = _lib.ctypes.c_int(0)
    fn = _lib.load_library().se_debug_get_option
    for name in (b"SE_S2POLY_PACK:48,0", b"SE_S2POLY_PACK:96,-1", b"SE_S2POLY_PACK:96,%d" % (38 * 96 * 32 + 96), b"SE_S2POLY_PACK:96",
                 b"SE_S2POLY_TABLE:5,0", b"SE_S2POLY_TABLE:0,7", b"SE_S2POLY_TABLE:0,0x"):
        assert fn(name, _lib.ctypes.byref(v)) == 1, name
    assert fn(b"SE_S2POLY_PACK:96,%d" % (38 * 96 * 32 + 95), _lib.ctypes.byref(v)) == 0
