"""The receiver's mode table and its per-call item counts, pinned to literals.

For every QRL_MODEM_* value qrl_demod_create accepts with use_mode_defaults = 1, at device_samp_rate 1 000 000 and 4 000 000 (batch 2,
max_chunk 40000), the values of qrl_demod_out_caps, qrl_demod_audio_cap and qrl_demod_time_domain_cap for n in {2, 1000, 40000}.  The
literals were recorded from the build BEFORE the two modem_type switches became one table and the five derivations of the counts one
function, so they pin the function and the table's family, kind and sps columns against the old code, not against themselves.  The caps do
not depend on filter_width, fm, m17 or lsb (2FSK2KFM and 2FSK2K, DMR and M17, USB and LSB have equal rows): those four columns are pinned by the
per-mode output tests, not here: every row's receiver runs against the oracle's chain with the row's literals in test_gpu_parity.py (the digital
modes, QRL_MODEM_QPSKVIDEO against QPSK250K's chain and handle; NBFM, AM, WBFM, SSB, DMR, M17 and BPSK8 in tests of their own there).  No kernel is
launched."""
import ctypes as C

import pytest

import qradiolink_amd as q

pytestmark = pytest.mark.gpu

NS = (2, 1000, 40000)
# modem_type: {device_samp_rate: one row per n of NS: (filtered_cap, constellation_cap, bits_cap, audio_cap, time_domain_cap)}
EXPECTED = {
    0: {   # QRL_MODEM_BPSK2K
        1000000: ((2, 8, 160, 0, 2), (22, 13, 160, 0, 102), (802, 208, 240, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (7, 9, 160, 0, 27), (202, 58, 160, 0, 1002)),
    },
    1: {   # QRL_MODEM_QPSK20K
        1000000: ((2, 8, 160, 0, 2), (42, 22, 160, 0, 102), (1602, 542, 640, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (12, 12, 160, 0, 27), (402, 142, 240, 0, 1002)),
    },
    2: {   # QRL_MODEM_QPSKVIDEO
        1000000: ((3, 11, 160, 0, 2), (502, 510, 640, 0, 102), (20002, 20010, 20160, 0, 4002)),
        4000000: ((3, 11, 160, 0, 2), (128, 136, 240, 0, 27), (5003, 5011, 5120, 0, 1002)),
    },
    3: {   # QRL_MODEM_4FSK2K
        1000000: ((2, 8, 160, 0, 2), (22, 10, 160, 0, 102), (802, 97, 240, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (7, 8, 160, 0, 27), (202, 30, 160, 0, 1002)),
    },
    4: {   # QRL_MODEM_4FSK10KFM
        1000000: ((2, 8, 160, 0, 2), (82, 19, 160, 0, 102), (3202, 465, 560, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (22, 11, 160, 0, 27), (802, 122, 240, 0, 1002)),
    },
    5: {   # QRL_MODEM_4FSK2KFM
        1000000: ((2, 8, 160, 0, 2), (22, 10, 160, 0, 102), (802, 97, 240, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (7, 8, 160, 0, 27), (202, 30, 160, 0, 1002)),
    },
    6: {   # QRL_MODEM_4FSK1KFM
        1000000: ((2, 8, 160, 0, 2), (12, 9, 160, 0, 102), (402, 52, 160, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (4, 8, 160, 0, 27), (102, 19, 160, 0, 1002)),
    },
    7: {   # QRL_MODEM_QPSK2K
        1000000: ((2, 8, 160, 0, 2), (12, 11, 160, 0, 102), (402, 108, 240, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (4, 9, 160, 0, 27), (102, 33, 160, 0, 1002)),
    },
    8: {   # QRL_MODEM_NBFM2500
        1000000: ((2, 8, 160, 4, 2), (22, 10, 160, 12, 102), (802, 97, 160, 324, 4002)),
        4000000: ((2, 8, 160, 4, 2), (7, 8, 160, 6, 27), (202, 30, 160, 84, 1002)),
    },
    9: {   # QRL_MODEM_NBFM5000
        1000000: ((2, 8, 160, 4, 2), (22, 10, 160, 12, 102), (802, 97, 160, 324, 4002)),
        4000000: ((2, 8, 160, 4, 2), (7, 8, 160, 6, 27), (202, 30, 160, 84, 1002)),
    },
    10: {   # QRL_MODEM_WBFM
        1000000: ((2, 8, 160, 4, 2), (202, 30, 160, 12, 102), (8002, 897, 560, 324, 4002)),
        4000000: ((2, 8, 160, 4, 2), (52, 13, 160, 6, 27), (2002, 230, 240, 84, 1002)),
    },
    11: {   # QRL_MODEM_USB2500
        1000000: ((2, 8, 160, 1030, 2), (10, 9, 160, 1038, 102), (322, 43, 160, 1350, 4002)),
        4000000: ((2, 8, 160, 1030, 2), (4, 8, 160, 1032, 27), (82, 17, 160, 1110, 1002)),
    },
    12: {   # QRL_MODEM_LSB2500
        1000000: ((2, 8, 160, 1030, 2), (10, 9, 160, 1038, 102), (322, 43, 160, 1350, 4002)),
        4000000: ((2, 8, 160, 1030, 2), (4, 8, 160, 1032, 27), (82, 17, 160, 1110, 1002)),
    },
    14: {   # QRL_MODEM_AM5000
        1000000: ((2, 8, 160, 4, 2), (22, 10, 160, 12, 102), (802, 97, 160, 324, 4002)),
        4000000: ((2, 8, 160, 4, 2), (7, 8, 160, 6, 27), (202, 30, 160, 84, 1002)),
    },
    15: {   # QRL_MODEM_2FSK2KFM
        1000000: ((2, 8, 160, 0, 2), (42, 12, 160, 0, 102), (1602, 186, 240, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (12, 9, 160, 0, 27), (402, 52, 160, 0, 1002)),
    },
    16: {   # QRL_MODEM_2FSK1KFM
        1000000: ((2, 8, 160, 0, 2), (22, 10, 160, 0, 102), (802, 97, 160, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (7, 8, 160, 0, 27), (202, 30, 160, 0, 1002)),
    },
    17: {   # QRL_MODEM_2FSK2K
        1000000: ((2, 8, 160, 0, 2), (42, 12, 160, 0, 102), (1602, 186, 240, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (12, 9, 160, 0, 27), (402, 52, 160, 0, 1002)),
    },
    18: {   # QRL_MODEM_2FSK1K
        1000000: ((2, 8, 160, 0, 2), (22, 10, 160, 0, 102), (802, 97, 160, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (7, 8, 160, 0, 27), (202, 30, 160, 0, 1002)),
    },
    19: {   # QRL_MODEM_2FSK10KFM
        1000000: ((2, 8, 160, 0, 2), (82, 35, 160, 0, 102), (3202, 1075, 640, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (22, 15, 160, 0, 27), (802, 275, 240, 0, 1002)),
    },
    20: {   # QRL_MODEM_GMSK2K
        1000000: ((2, 8, 160, 0, 2), (42, 12, 160, 0, 102), (1602, 186, 240, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (12, 9, 160, 0, 27), (402, 52, 160, 0, 1002)),
    },
    21: {   # QRL_MODEM_GMSK1K
        1000000: ((2, 8, 160, 0, 2), (22, 10, 160, 0, 102), (802, 97, 160, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (7, 8, 160, 0, 27), (202, 30, 160, 0, 1002)),
    },
    22: {   # QRL_MODEM_GMSK10K
        1000000: ((2, 8, 160, 0, 2), (82, 35, 160, 0, 102), (3202, 1075, 640, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (22, 15, 160, 0, 27), (802, 275, 240, 0, 1002)),
    },
    24: {   # QRL_MODEM_BPSK1K
        1000000: ((2, 8, 160, 0, 2), (22, 10, 160, 0, 102), (802, 97, 160, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (7, 8, 160, 0, 27), (202, 30, 160, 0, 1002)),
    },
    25: {   # QRL_MODEM_BPSK8
        1000000: ((2, 8, 160, 0, 2), (22, 10, 160, 0, 102), (802, 97, 160, 0, 4002)),
        4000000: ((2, 8, 160, 0, 2), (7, 8, 160, 0, 27), (202, 30, 160, 0, 1002)),
    },
    26: {   # QRL_MODEM_QPSK250K
        1000000: ((3, 11, 160, 0, 2), (502, 510, 640, 0, 102), (20002, 20010, 20160, 0, 4002)),
        4000000: ((3, 11, 160, 0, 2), (128, 136, 240, 0, 27), (5003, 5011, 5120, 0, 1002)),
    },
    27: {   # QRL_MODEM_4FSK100K
        1000000: ((3, 8, 160, 0, 2), (502, 133, 240, 0, 102), (20002, 5008, 5120, 0, 4002)),
        4000000: ((3, 8, 160, 0, 2), (128, 40, 160, 0, 27), (5003, 1258, 1360, 0, 1002)),
    },
    40: {   # QRL_MODEM_M17
        1000000: ((2, 8, 24, 0, 2), (26, 14, 36, 0, 102), (962, 248, 504, 0, 4002)),
        4000000: ((2, 8, 24, 0, 2), (8, 10, 28, 0, 27), (242, 68, 144, 0, 1002)),
    },
    41: {   # QRL_MODEM_DMR
        1000000: ((2, 8, 24, 0, 2), (26, 14, 36, 0, 102), (962, 248, 504, 0, 4002)),
        4000000: ((2, 8, 24, 0, 2), (8, 10, 28, 0, 27), (242, 68, 144, 0, 1002)),
    },
}
REFUSED = (13, 23, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63)   # every other value of 0 .. 63 (13 = QRL_MODEM_CW600USB is a transmitter mode)


def _create(ctx, modem_type, rate):
    cfg = q._Config()
    cfg.modem_type, cfg.use_mode_defaults, cfg.device_samp_rate = modem_type, 1, rate
    cfg.batch, cfg.max_chunk, cfg.enable_side_outputs = 2, 40000, 1
    h = C.c_void_p()
    return ctx.lib.qrl_demod_create(ctx.h, C.byref(cfg), C.byref(h)), h


def test_mode_table_and_call_counts(qrl_ctx):
    lib = qrl_ctx.lib
    for mt, per_rate in EXPECTED.items():
        for rate, rows in per_rate.items():
            rc, h = _create(qrl_ctx, mt, rate)
            assert rc == 0, (mt, rate, lib.qrl_last_error().decode())
            try:
                for n, want in zip(NS, rows):
                    f, c, b, a, t = (C.c_size_t() for _ in range(5))
                    assert lib.qrl_demod_out_caps(h, n, C.byref(f), C.byref(c), C.byref(b)) == 0
                    assert lib.qrl_demod_audio_cap(h, n, C.byref(a)) == 0
                    assert lib.qrl_demod_time_domain_cap(h, n, C.byref(t)) == 0
                    got = (f.value, c.value, b.value, a.value, t.value)
                    assert got == want, (mt, rate, n, got, want)
            finally:
                lib.qrl_demod_destroy(h)
    for mt in REFUSED:
        rc, h = _create(qrl_ctx, mt, 1000000)
        assert rc == -1 and not h.value, (mt, rc)   # QRL_ERR_ARG
        assert lib.qrl_last_error() == b"modem_type not supported by this build"
