"""QRL_OPT_SC16_BASEBAND at the C ABI and in the Python binding, on the CPU: include/qrl_hip.h gives the option the value 6 and says in front of
qrl_demod_process_sc16 what a 1 Msps handle now does, the binding has the constant and Demod.enable_sc16_baseband, and a NULL handle is
QRL_ERR_ARG before any device work."""
import inspect
import os
import re

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRL_ERR_ARG = -1


def _header():
    return open(os.path.join(ROOT, "include", "qrl_hip.h")).read()


def test_header_gives_the_option_the_value_6():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"enum\s*\{([^}]*\bQRL_OPT_OVERLAP\b[^}]*)\}", code)
    assert m, "no enum with the per-handle options"
    values = dict(re.findall(r"\b(QRL_OPT_\w+)\s*=\s*(\d+)", m.group(1)))
    assert values["QRL_OPT_SC16_BASEBAND"] == "6"
    assert len(set(values.values())) == len(values)           # no value is taken twice
    assert values["QRL_OPT_INPUT_RESIDENT"] == "5" and values["QRL_OPT_OVERLAP"] == "1"


def test_header_comment_says_what_a_1_msps_handle_does_now():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+qrl_demod_process_sc16\s*\(", _header(), flags=re.S)
    assert m, "no comment in front of qrl_demod_process_sc16"
    for word in ("k_resamp", "k_dec2_fir", "QRL_ERR_ARG", "32768", "QRL_OPT_SC16_BASEBAND"):
        assert word in m.group(1), word
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*enum\s*\{\s*QRL_OPT_OVERLAP", _header(), flags=re.S)
    assert m and "QRL_OPT_SC16_BASEBAND (default 0)" in m.group(1)


def test_python_binding_has_the_constant_and_the_method():
    assert q.OPT_SC16_BASEBAND == 6
    assert callable(q.Demod.enable_sc16_baseband)
    assert inspect.signature(q.Demod.enable_sc16_baseband).parameters["on"].default is True
    assert "enable_sc16_baseband" in q.Demod.process_sc16_async.__doc__ and "1 Msps" in q.Demod.process_sc16_async.__doc__


def test_null_handle_is_an_arg_error():
    lib = q.load_library()
    assert lib.qrl_demod_set_option(None, q.OPT_SC16_BASEBAND, 1) == QRL_ERR_ARG
    assert lib.qrl_demod_set_option(None, q.OPT_SC16_BASEBAND, 0) == QRL_ERR_ARG
