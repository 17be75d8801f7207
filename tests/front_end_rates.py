"""The device-rate front ends by decimation D = device_samp_rate / 1e6 (filter: low_pass(1, rate, 480e3, 100e3, BLACKMAN_HARRIS),
about 41.8 D taps = 42 taps per phase for every D): which summation contract of the oracle defines a rate, and which kernel the library
runs for it.  Written out by hand from docs/KERNELS.md 17, NOT derived from the selection rules: test_oracle.py pins the oracle's rules
(orc_decim_uses_*) against it on the CPU, test_gpu_front_end_rates.py the kernel the library reports on the GPU."""

# kernel names as qrl_demod_profile_read reports them
GENERIC, M16, PM, PL = "k_decim", "k_decim_mfma", "k_decim_pm", "k_decim_plx"

FIRST_D, LAST_D = 2, 183          # 184:1 and beyond: the generic tile ((832 + 107 D) * 8 bytes) no longer fits the 160 KiB of a CU
PM_NS = (3, 5, 7, 13, 25)         # phase slabs (steps of four phases) the pm kernel is instantiated for: NS = ceil(D / 4)

_PM = set(range(9, 13)) | set(range(17, 21)) | set(range(25, 29)) | set(range(49, 53)) | set(range(97, 101))
_PL = (set(range(66, 97, 2)) | set(range(102, 129, 2))) - _PM
_M16 = ({8} | set(range(13, 17)) | set(range(21, 25)) | set(range(29, 49)) | set(range(53, 66)) | set(range(67, 114, 2))) - _PM
_GENERIC = set(range(2, 8)) | set(range(115, 128, 2)) | set(range(129, LAST_D + 1))


def front_end_class(D):
    """GENERIC, M16, PM or PL for D in FIRST_D .. LAST_D"""
    hits = [name for name, s in ((GENERIC, _GENERIC), (M16, _M16), (PM, _PM), (PL, _PL)) if D in s]
    assert len(hits) == 1, (D, hits)
    return hits[0]


def generic_lds_bytes(D):
    """dynamic LDS of the generic kernel's tile for a front-end filter (decim_lds_bytes): k_decim<4, 44> below 8:1, k_decim<1, 14> above"""
    R, Jpad = (4, 44) if D < 8 else (1, 42)
    W = 64 * R + Jpad
    PT = (R * ((W + R - 1) // R)) | 1
    return (512 + 64 + 4 * 64 * R + D * PT) * 8
