"""s2p_decoded_to_frames (csrc/replay.hip, SPEC.md N3o) without a device: the export, the pinned library version and every refusal
of include/s2p_hip.h, each of which happens before any launch."""
import os

from s2p_amd import _lib

NAME = "s2p_decoded_to_frames"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_hand_off_at_version_125():
    L = _lib.lib()
    assert hasattr(L, NAME) and NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME]) == 10
    assert L.s2p_version() == 125
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    assert "int %s(int dtype, const void* y, int y_pitch, int64_t pixels_total, int C, int quantize, void* x, int x_pitch," % NAME in header
    assert "#define S2P_VERSION 125" in header


def _call(dtype=0, y=4096, y_pitch=4, pixels=8, C=3, quantize=1, x=8192, x_pitch=4, u8=12288):
    # non-NULL, 16-byte aligned addresses that are never dereferenced: every refusal happens before any launch
    return _lib.lib().s2p_decoded_to_frames(dtype, y, y_pitch, pixels, C, quantize, x, x_pitch, u8, None)


def test_refusals_happen_before_any_launch():
    L = _lib.lib()
    cases = {"bad dtype": dict(dtype=7), "null y": dict(y=None), "both outputs null": dict(x=None, u8=None), "C < 1": dict(C=0),
             "negative C": dict(C=-3), "C > y_pitch": dict(C=5, x_pitch=8), "C > x_pitch": dict(C=5, y_pitch=8),
             "negative pixels_total": dict(pixels=-1), "negative y_pitch": dict(y_pitch=-4), "negative x_pitch": dict(x_pitch=-4),
             "misaligned x": dict(x=8192 + 8), "misaligned x, bf16": dict(dtype=1, y_pitch=8, x_pitch=8, x=8192 + 2),
             "misaligned y": dict(y=4096 + 2)}
    for name, kw in cases.items():
        rc = _call(**kw)
        msg = L.s2p_last_error().decode()
        assert rc != 0 and msg.startswith(NAME + ":"), (name, rc, msg)


def test_an_empty_batch_is_a_no_op_that_looks_at_no_pointer():
    assert _call(pixels=0, y=None, x=None, u8=None) == 0
    assert _call(dtype=1, pixels=0, y=None, x=None, u8=None, y_pitch=8, x_pitch=8) == 0
