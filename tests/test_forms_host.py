"""The rule that chooses a gated convolution's kernel form, checked on the host: choose_form / layer_facts
(sketchedit_amd/csrc/se_dispatch.h) through se_debug_gconv_form, against the table of tests/forms_util.py.

The rule is integer arithmetic on the layer, the sizes, the mode and the developer switches: no device is needed to ask it, and
run_gconv launches what the same function answers (tests/test_gpu_forms.py holds the answer against the launches recorded on
the GPU).  A condition narrowed or widened by mistake fails here at the row of the form, or of the neighbour that must take over.
"""
import pytest

from sketchedit_amd import _lib
import forms_util as FU


_forms = FU.predict


def _set(seopt, r):
    for name, v in r.switches.items():
        seopt.set(name, v)


CASES = FU.cases()


@pytest.mark.parametrize("case", CASES, ids=[FU.row_id(r, s) for r, s in CASES])
def test_every_row_gives_its_form_at_every_batch(case, seopt):
    """list(row.pre) + [row.form] at the table's batch, and the same at B = 1, 2 and 3 (the choice ignores the batch)."""
    r, shape = case
    _set(seopt, r)
    want = list(r.pre) + [r.form]
    assert _forms(r, shape) == want
    for B in (1, 2, 3):
        assert _forms(r, shape, B=B) == want, B


@pytest.mark.parametrize("t", FU.LL_THRESHOLDS, ids=[FU.row_id(t.row) for t in FU.LL_THRESHOLDS])
def test_low_latency_thresholds(t, seopt):
    """With the switch at the workgroup (tile) count per image of the row's last shape the row's form runs, one above it the
    small-grid gather-GEMM -- at every batch."""
    r, shape = t.row, t.row.shapes[-1]
    mode = "bf16-lowlat" if r.mode == "bf16" else "lowlat"
    _set(seopt, r)
    for B in (1, 2, 3):
        seopt.set(t.switch, t.count)
        assert _forms(r, shape, B=B, mode=mode) == list(r.pre) + [r.form], B
        seopt.set(t.switch, t.count + 1)
        assert _forms(r, shape, B=B, mode=mode) == [t.below], B


def test_conservative_and_net_select_the_f43_mode(seopt):
    """SE_WINOGRAD_F43: 1 the hybrid kernel everywhere, 2 netG only, 0 nowhere; SE_FLAG_CONSERVATIVE is mode 2 for the call."""
    def ask(net, conservative=False):
        return _lib.gconv_form(96, 192, 8, 8, net=net, conservative=conservative)
    assert ask(_lib.SE_NET_G) == ask(_lib.SE_NET_M) == ask(_lib.SE_NET_G, True) == ["wino24"]
    assert ask(_lib.SE_NET_M, True) == ["wino"]
    seopt.set("SE_WINOGRAD_F43", 2)
    assert ask(_lib.SE_NET_G) == ["wino24"] and ask(_lib.SE_NET_M) == ["wino"]
    seopt.set("SE_WINOGRAD_F43", 0)
    assert ask(_lib.SE_NET_G) == ask(_lib.SE_NET_M) == ["wino"]
    assert _lib.gconv_form(48, 192, 8, 8) == ["gconv_n192"]              # (wino24_c48 has no F(2x2,3x3) form behind it)


# layer_facts, one layer of each packing rule: (cin, cin1, vector, cout, k, stride, rate, up) -> per image the layer must have, a
# call (H, W, bf16) that reaches the form which reads it, and that form.  A flag lost from layer_facts turns the call into the
# gather-GEMM (or the next form down); pack_layer_images checks the images it built against the same flags.
FACTS = [
    ("96to192", (96, 0, 0, 192, 3, 1, 1, 0), [("u24 ub24", 2, 4, 0, ["wino24"]), ("u", 2, 2, 0, ["wino"]), ("w16s", 12, 12, 1, ["rconv16"])]),
    ("192to192-tensor", (96, 96, 0, 192, 3, 1, 1, 0), [("u24b ub24", 2, 4, 0, ["wino24_2src"]), ("u", 2, 2, 0, ["wino_2src"])]),
    ("192to192-vector", (96, 96, 1, 192, 3, 1, 1, 0), [("wv u24", 2, 4, 0, ["vecbias", "wino24"]), ("wv u1", 2, 2, 0, ["vecbias", "wino"]),
                                                         ("wv16 w16s", 12, 12, 1, ["vecbias", "rconv16"])]),
    ("48to192", (48, 0, 0, 192, 3, 1, 1, 0), [("u24 ub24", 2, 4, 0, ["wino24_c48"]), ("no w16s", 12, 12, 1, ["gconv_n192_bf16"])]),
    ("48to96", (48, 0, 0, 96, 3, 1, 1, 0), [("u ub", 2, 2, 0, ["wino48"]), ("w96", 12, 12, 1, ["rconv96"])]),
    ("24to96", (24, 0, 0, 96, 3, 1, 1, 0), [("u ub", 2, 2, 0, ["wino48_c24"]), ("w96", 12, 12, 1, ["rconv96_c24"])]),
    ("24to24", (24, 0, 0, 24, 3, 1, 1, 0), [("wx2", 2, 2, 0, ["rtilew2"]), ("wx", 3, 2, 0, ["rtilew"]), ("direct, NP 32", 3, 3, 0, ["rtile"]),
                                            ("direct bf16", 3, 3, 1, ["rtile_bf16"])]),
    ("24to24-d2", (24, 0, 0, 24, 3, 1, 2, 0), [("no wx", 4, 4, 0, ["gconv_n24"])]),
    ("96to96-up", (96, 0, 0, 96, 3, 1, 1, 1), [("u ub", 2, 2, 0, ["winoup"]), ("w96", 12, 12, 1, ["rconv96_up"])]),
    ("48to48-up", (48, 0, 0, 48, 3, 1, 1, 1), [("u ub", 2, 2, 0, ["winoup48"]), ("no w96", 12, 12, 1, ["rtile_bf16_up2"])]),
    ("24to96-s2", (24, 0, 0, 96, 3, 2, 1, 0), [("w96", 12, 12, 1, ["rconv96_s2"]), ("no u", 12, 12, 0, ["gconv_n96"])]),
    ("48to96-s2", (48, 0, 0, 96, 3, 2, 1, 0), [("no w96", 12, 12, 1, ["gconv_n96_bf16"])]),
    ("3to48-k5", (3, 0, 0, 48, 5, 1, 1, 0), [("wdw", 9, 18, 0, ["rtile_dense5w"]), ("wd", 9, 17, 0, ["rtile_dense5"]), ("w16d", 9, 17, 1, ["rtile_bf16_d4"])]),
    ("4to48-k5", (4, 0, 0, 48, 5, 1, 1, 0), [("wdw", 9, 18, 0, ["rtile_dense5w"]), ("wd", 9, 17, 0, ["rtile_dense5"]), ("w16d", 9, 17, 1, ["rtile_bf16_d4"])]),
    ("5to48-k5", (5, 0, 0, 48, 5, 1, 1, 0), [("wdw", 9, 18, 0, ["rtile_dense5w"]), ("wd", 9, 17, 0, ["rtile_dense5"]), ("no w16d", 9, 17, 1, ["rtile_bf16"])]),
    ("8to48-k5", (8, 0, 0, 48, 5, 1, 1, 0), [("no wd: every stored channel is real", 9, 18, 0, ["rtile"])]),
]


@pytest.mark.parametrize("name,layer,calls", FACTS, ids=[f[0] for f in FACTS])
def test_layer_facts_reach_the_form_that_reads_each_image(name, layer, calls):
    cin, cin1, vec, cout, k, stride, rate, up = layer
    for what, H, W, bf, want in calls:
        got = _lib.gconv_form(cin, cout, H, W, k=k, stride=stride, rate=rate, upsample=bool(up), cin1=cin1, x1_is_vector=bool(vec), bf16=bool(bf))
        assert got == want, (name, what, got)


def test_bad_layers_and_small_buffers_are_refused():
    import ctypes
    lib = _lib.load_library()
    buf = ctypes.create_string_buffer(64)
    ok = lambda *a: lib.se_debug_gconv_form(*a)      # noqa: E731
    # cin cin1 vec cout k stride rate act up B H W flags net
    assert ok(96, 0, 0, 192, 3, 1, 1, 0, 0, 1, 8, 8, 0, 0, buf, 64) == 0 and buf.value == b"wino24"
    assert ok(96, 0, 0, 192, 3, 1, 1, 0, 0, 1, 8, 8, 0, 0, buf, 6) == 1                   # "wino24" needs 7 bytes
    assert ok(96, 96, 1, 192, 3, 1, 1, 0, 0, 1, 8, 8, 0, 0, buf, 14) == 1                 # "vecbias,wino24" needs 15
    assert ok(96, 96, 1, 192, 3, 1, 1, 0, 0, 1, 8, 8, 0, 0, buf, 15) == 0 and buf.value == b"vecbias,wino24"
    assert ok(96, 0, 0, 196, 3, 1, 1, 0, 0, 1, 8, 8, 0, 0, buf, 64) == 1                  # Cout % 8
    assert ok(96, 0, 0, 400, 3, 1, 1, 0, 0, 1, 8, 8, 0, 0, buf, 64) == 1                  # no configuration that wide
    assert ok(94, 96, 0, 192, 3, 1, 1, 0, 0, 1, 8, 8, 0, 0, buf, 64) == 1                 # two sources: whole granules
    assert ok(12, 0, 0, 3, 5, 1, 1, 2, 0, 1, 8, 8, 0, 0, buf, 64) == 1                    # raw conv: 3x3 12 -> {1, 3} only
    assert ok(12, 0, 0, 3, 3, 1, 1, 2, 0, 1, 8, 8, 0, 0, None, 64) == 1
    assert ok(12, 0, 0, 3, 3, 1, 1, 2, 0, 1, 8, 8, 0, 0, buf, 64) == 0 and buf.value == b"small_conv"
