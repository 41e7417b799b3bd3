"""CPU: capi.knobs is the one way to flip a QE_* knob in a live process -- the library sees the knob inside the block and no
longer after it, also when the body raised, and a variable that was set before the block gets its old value back.  Seen through
the host-only query qe_quantconv2d_float_input_path, whose only knob is QE_F32_MFMA."""
import ctypes
import os

import pytest

from quantize_amd import capi


def _path():
    sh = capi.conv_shape(2, 64, 14, 14, 64, 3, 3, 1, 1)
    wq = capi.QeQParam(None, 8, 1, None, None, 1)           # the query reads no operand
    return int(capi.lib().qe_quantconv2d_float_input_path(ctypes.byref(sh), ctypes.byref(wq)))


def test_knobs_set_and_restore():
    assert os.environ.get("QE_F32_MFMA") is None
    assert _path() == 1
    with capi.knobs(QE_F32_MFMA="0"):
        assert os.environ["QE_F32_MFMA"] == "0"
        assert _path() == 0
    assert os.environ.get("QE_F32_MFMA") is None
    assert _path() == 1


def test_knobs_restore_after_an_exception():
    with pytest.raises(ZeroDivisionError):
        with capi.knobs(QE_F32_MFMA="0"):
            assert _path() == 0
            1 / 0
    assert os.environ.get("QE_F32_MFMA") is None
    assert _path() == 1


def test_knobs_keep_a_value_set_before_the_block():
    with capi.knobs(QE_F32_MFMA="0"):                       # stands for a variable of the caller's environment
        with capi.knobs(QE_F32_MFMA=None):                  # None: unset
            assert "QE_F32_MFMA" not in os.environ
            assert _path() == 1
        assert os.environ["QE_F32_MFMA"] == "0"
        assert _path() == 0
        with capi.knobs(QE_F32_MFMA=1):                     # values are written as strings
            assert os.environ["QE_F32_MFMA"] == "1"
            assert _path() == 1
        assert os.environ["QE_F32_MFMA"] == "0"
        assert _path() == 0
    assert _path() == 1
