"""Per-stream carrier offsets at the C ABI, on CPU: the header declares qrl_{demod,mod,amod}_set_carrier_offsets, libqrl_hip.so
exports them, a NULL handle or a NULL array is QRL_ERR_ARG before any device work, and the Python methods check the length first."""
import ctypes as C
import math
import os
import re

import pytest

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["qrl_demod_set_carrier_offsets", "qrl_mod_set_carrier_offsets", "qrl_amod_set_carrier_offsets"]
QRL_ERR_ARG = -1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qrl_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_per_stream_setter(name):
    kind = name.split("_")[1]
    pat = r"\bint\s+%s\s*\(\s*qrl_%s\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*\)\s*;" % (name, kind)
    assert re.search(pat, _header()), "%s is not declared as int %s(qrl_%s*, const double*)" % (name, name, kind)


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_per_stream_setter(name):
    lib = q.load_library()
    assert hasattr(lib, name)
    assert name in q.EXPORTED_SYMBOLS


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_and_null_array_are_arg_errors(name):
    lib = q.load_library()
    fn = getattr(lib, name)
    hz = (C.c_double * 4)(0.0, 1200.0, -1200.0, 25000.0)
    assert fn(None, None) == QRL_ERR_ARG
    assert fn(None, hz) == QRL_ERR_ARG


@pytest.mark.parametrize("cls", [q.Demod, q.Mod, q.AMod])
def test_python_setter_checks_length_before_the_library(cls):
    class _NoLib:
        def __getattr__(self, n):
            raise AssertionError("the library was called (%s)" % n)

    obj = cls.__new__(cls)   # no handle, no device: the length check must come first
    obj.lib, obj.h, obj.batch = _NoLib(), None, 4
    with pytest.raises(ValueError):
        obj.set_carrier_offsets([0.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        obj.set_carrier_offsets([0.0] * 5)


def test_python_setter_passes_non_finite_values_to_the_library_check():
    """A NaN is no length error: it reaches the library, whose QRL_ERR_ARG becomes a QrlError (NULL handle here)."""
    obj = q.Demod.__new__(q.Demod)
    obj.lib, obj.h, obj.batch = q.load_library(), None, 2
    with pytest.raises(q.QrlError):
        obj.set_carrier_offsets([0.0, math.nan])
