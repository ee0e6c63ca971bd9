"""The rule that decides whether a pass of the default mode runs as two half-batch chains (pair_rule, sketchedit_amd/csrc/se_host.h;
DESIGN.md section 6), asked on the host through the "SE_PAIR_RULE:B,H,W,flags" entry of se_debug_get_option: integer arithmetic on the pass and SE_PAIR_MIN_PIXELS, no
device.  tests/test_gpu_pairs.py holds the results of paired calls against unpaired ones; tools/pair_host_check.hip walks the
rule and the dry-run plans of paired passes under the host sanitizers."""
import pytest

from sketchedit_amd import _lib


def test_default_threshold_is_documented_value():
    """2^21 pixels, or 0 where the measurement refused the pairing: nothing in between ships"""
    assert _lib.get_option("SE_PAIR_MIN_PIXELS") in (0, 1 << 21)


@pytest.mark.parametrize("threshold", [1, 4096, 1 << 20, 1 << 21, 1 << 22])
def test_both_sides_of_the_threshold(seopt, threshold):
    seopt.set("SE_PAIR_MIN_PIXELS", threshold)
    # (B, H, W) with B H W == threshold where the threshold allows one, and one image / row / column fewer
    at = [(B, H, W) for B, H, W in [(2, 8, threshold // 16), (4, 16, threshold // 64), (3, 16, 16), (5, 64, 64), (32, 256, 256), (8, 512, 512)]
          if W >= 1 and B * H * W >= threshold]
    assert at
    for B, H, W in at:
        assert _lib.pair_rule(B, H, W), (B, H, W)
        assert not _lib.pair_rule(B, H, W, low_latency=True), (B, H, W)
        assert not _lib.pair_rule(1, B * H, W), (B, H, W)                 # one image is never paired, however large
    below = [(2, 8, threshold // 16 - 1), (2, 7, threshold // 16), (3, 16, (threshold - 1) // 48)]
    for B, H, W in below:
        if H >= 1 and W >= 1 and B * H * W < threshold:
            assert not _lib.pair_rule(B, H, W), (B, H, W)
    if threshold >= 48:
        assert any(H >= 1 and W >= 1 and B * H * W < threshold for B, H, W in below)


def test_exactly_at_the_threshold(seopt):
    seopt.set("SE_PAIR_MIN_PIXELS", 3 * 40 * 72)
    assert _lib.pair_rule(3, 40, 72) and not _lib.pair_rule(3, 40, 71) and not _lib.pair_rule(2, 40, 72)
    seopt.set("SE_PAIR_MIN_PIXELS", 3 * 40 * 72 + 1)
    assert not _lib.pair_rule(3, 40, 72) and _lib.pair_rule(5, 40, 72)      # odd batches pair like even ones


def test_zero_is_never(seopt):
    seopt.set("SE_PAIR_MIN_PIXELS", 0)
    for B, H, W in [(2, 16, 16), (5, 64, 64), (32, 256, 256), (64, 512, 512)]:
        assert not _lib.pair_rule(B, H, W) and not _lib.pair_rule(B, H, W, low_latency=True)
    seopt.set("SE_PAIR_MIN_PIXELS", -5)
    assert not _lib.pair_rule(32, 256, 256)


def test_the_query_adds_no_option_and_no_symbol():
    """the rule is asked through se_debug_get_option's derived entry: it cannot be set, and malformed queries are refused"""
    lib = _lib.load_library()
    assert lib.se_debug_set_option(b"SE_PAIR_RULE:4,64,64,0", 1) != 0
    import ctypes
    v = ctypes.c_int(7)
    for bad in (b"SE_PAIR_RULE:", b"SE_PAIR_RULE:4,64,64", b"SE_PAIR_RULE:4,64,64,0,1", b"SE_PAIR_RULE:4,64,x,0", b"SE_PAIR_RULE:4,0,64,0"):
        assert lib.se_debug_get_option(bad, ctypes.byref(v)) != 0 and v.value == 7, bad


def test_bad_arguments():
    with pytest.raises(_lib.SketchEditHipError):
        _lib.pair_rule(0, 64, 64)
