"""QRL_OPT_IQ8_BASEBAND at the C ABI and in the Python binding, on the CPU: include/qrl_hip.h gives the option the value 7 and documents it
beside QRL_OPT_SC16_BASEBAND and in front of qrl_demod_process_sc8, the binding has the constant and Demod.enable_iq8_baseband, the
process_sc8 / process_cu8 docstrings say when a 1 Msps handle takes them, and a NULL handle is QRL_ERR_ARG before any device work."""
import inspect
import os
import re

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRL_ERR_ARG = -1


def _header():
    return open(os.path.join(ROOT, "include", "qrl_hip.h")).read()


def test_header_gives_the_option_the_value_7():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"enum\s*\{([^}]*\bQRL_OPT_OVERLAP\b[^}]*)\}", code)
    assert m, "no enum with the per-handle options"
    values = dict(re.findall(r"\b(QRL_OPT_\w+)\s*=\s*(\d+)", m.group(1)))
    assert values["QRL_OPT_IQ8_BASEBAND"] == "7"
    assert len(set(values.values())) == len(values)           # no value is taken twice
    assert values["QRL_OPT_SC16_BASEBAND"] == "6" and values["QRL_OPT_INPUT_RESIDENT"] == "5" and values["QRL_OPT_OVERLAP"] == "1"


def test_header_documents_the_option_beside_sc16_baseband():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*enum\s*\{\s*QRL_OPT_OVERLAP", _header(), flags=re.S)
    assert m, "no comment in front of the options"
    text = m.group(1)
    assert "QRL_OPT_IQ8_BASEBAND (default 0)" in text and "QRL_OPT_SC16_BASEBAND (default 0)" in text
    assert text.index("QRL_OPT_SC16_BASEBAND (default 0)") < text.index("QRL_OPT_IQ8_BASEBAND (default 0)")
    for word in ("qrl_demod_process_sc8", "_host", "QRL_ERR_ARG", "independent", "multiple of 8 samples"):
        assert word in text[text.index("QRL_OPT_IQ8_BASEBAND (default 0)"):], word


def test_header_comment_says_when_a_1_msps_handle_takes_8_bit_calls():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+qrl_demod_process_sc8\s*\(", _header(), flags=re.S)
    assert m, "no comment in front of qrl_demod_process_sc8"
    for word in ("QRL_OPT_IQ8_BASEBAND", "1 Msps", "k_resamp", "k_dec2_fir", "untuned", "QRL_ERR_ARG"):
        assert word in m.group(1), word


def test_python_binding_has_the_constant_and_the_method():
    assert q.OPT_IQ8_BASEBAND == 7
    assert q.OPT_SC16_BASEBAND == 6
    assert callable(q.Demod.enable_iq8_baseband)
    assert inspect.signature(q.Demod.enable_iq8_baseband).parameters["on"].default is True
    for method in (q.Demod.process_sc8, q.Demod.process_cu8, q.Demod.process_sc8_async, q.Demod.process_cu8_async):
        assert "enable_iq8_baseband" in method.__doc__ and "1 Msps" in method.__doc__, method.__name__


def test_null_handle_is_an_arg_error():
    lib = q.load_library()
    assert lib.qrl_demod_set_option(None, 7, 1) == QRL_ERR_ARG
    assert lib.qrl_demod_set_option(None, q.OPT_IQ8_BASEBAND, 0) == QRL_ERR_ARG
