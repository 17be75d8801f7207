"""DMR receive call layer on the CPU: qradiolink_amd/csrc/dmr_rx_core.hpp, the code k_dmr_rx calls, against the recorded call records of
tests/golden/ref/dmr_rx.npz byte for byte, and against the live reference where it is present (its DMRControl, compiled unmodified, one
addFrames call per burst: tests/host/dmr_rx_ref.cpp); embedded_lc_decode against CDMREmbeddedData under every single and 2 000 double bit
errors; the bound of the alias buffer; and the same core under the address and undefined-behaviour sanitizers
(tests/host/test_dmr_rx_core.cpp)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dmr_l2
import dmr_rx
import dmr_tx

ROOT = dmr_rx.ROOT
G = dmr_rx.load_golden()
NAMES = list(G["names"])


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return dmr_rx.load_core(tmp_path_factory.mktemp("dmr_rx_core"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    r = dmr_rx.load_ref(tmp_path_factory.mktemp("dmr_rx_ref"))
    if r is None:
        pytest.skip("the reference's sources / oracle/_ref/libqrl_ref.so are not here")
    return r


@pytest.fixture(scope="module")
def tx_ref(tmp_path_factory):
    r = dmr_tx.load_ref(tmp_path_factory.mktemp("dmr_tx_ref"))
    if r is None:
        pytest.skip("the reference's sources / oracle/_ref/libqrl_ref.so are not here")
    return r


def _run_core(core, name):
    """a scenario through the core, its configuration switched where the scenario says; -> (records, layer-2 records, most alias bytes held)"""
    _, inp, _, cc, prom, reconfig = dmr_rx.scenario(G, name)
    cuts = [0] + [slot for slot, _, _ in reconfig] + [inp.shape[0]]
    cfgs = [(cc, prom)] + [(c, p) for _, c, p in reconfig]
    out, l2, state, most = [], [], None, 0
    for (a, b), (c, p) in zip(zip(cuts[:-1], cuts[1:]), cfgs):
        o, l, state, m = core.run(inp[a:b], c, p, state)
        out.append(o)
        l2.append(l)
        most = max(most, m)
    return np.concatenate(out), np.concatenate(l2), most


@pytest.mark.parametrize("name", NAMES)
def test_core_equals_the_golden(core, name):
    _, inp, want, _, _, _ = dmr_rx.scenario(G, name)
    got, l2, _ = _run_core(core, name)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "bursts %s differ; first: core %s, reference %s" % (bad[:8], got[bad[0], :36], want[bad[0], :36])
    # the layer-2 records the core was fed are those of the independent restatement of tests/dmr_l2.py
    for i in range(0, inp.shape[0], 7):
        assert bytes(l2[i]) == bytes(dmr_l2.record(inp[i].tobytes(), dmr_rx.AUDIO_FEC)), "layer-2 record %d" % i


def test_core_cut_at_every_burst_equals_the_uncut_run(core):
    """the state carried through its 128 bytes from burst to burst"""
    for name in NAMES:
        _, inp, want, cc, prom, reconfig = dmr_rx.scenario(G, name)
        if reconfig:
            continue
        state, rows = None, []
        for i in range(inp.shape[0]):
            o, _, state, _ = core.run(inp[i:i + 1], cc, prom, state)
            rows.append(o[0])
        assert np.array_equal(np.stack(rows), want), name


def test_golden_is_fresh(ref, tx_ref):
    g = dmr_rx.record_golden(ref, tx_ref)
    assert sorted(g) == sorted(G)
    for k in g:
        assert np.array_equal(g[k], G[k]), k


def test_core_equals_the_live_reference_on_shuffled_streams(core, ref):
    """bursts of the golden scenarios in an order no scenario has: every fifth burst dropped, then pairs swapped"""
    for name in ("whole_call", "damaged_fragments", "alias_corners", "promiscuous_lock", "data"):
        _, inp, _, cc, prom, _ = dmr_rx.scenario(G, name)
        for mode in (0, 1):
            keep = [i for i in range(inp.shape[0]) if i % 5 != 4]
            x = inp[keep].copy()
            m = (x.shape[0] - 3) // 4 * 4
            x[1:m + 1:4], x[2:m + 2:4] = x[2:m + 2:4].copy(), x[1:m + 1:4].copy()
            if mode:
                x = x[::-1].copy()
            got, _, _, _ = core.run(x, cc, prom ^ mode)
            want = ref.run(x, cc, prom ^ mode)
            assert np.array_equal(got, want), (name, mode)


def _corrupt(frag, positions):
    f = list(frag)
    for p in positions:
        f[p // 32] ^= 1 << (31 - p % 32)
    return f


def _check_embedded(core, ref, frag):
    ok, flco, data = ref.embedded(frag)
    code, mine = core.embedded(frag)
    assert (code == 3) == ok, (frag, code, ok)
    if ok:
        assert mine == data and (mine[0] & 0x3F) == flco
    elif code == 2:
        assert mine == data          # the reference has written m_data before it checks the sum
    else:
        assert mine == bytes(9) and data == bytes(9)
    return code


def test_embedded_lc_decode_equals_the_reference_under_bit_errors(core, ref):
    rng = np.random.RandomState(77)
    codes = {0: 0, 1: 0, 2: 0, 3: 0}
    for trial in range(4):
        lc9 = bytes(rng.randint(0, 256, 9).astype(np.uint8))
        frag = dmr_rx.matrix_fragments(dmr_rx.embedded_matrix(lc9))
        assert _check_embedded(core, ref, frag) == 3 and core.embedded(frag)[1] == lc9
        for p in range(128):
            code = _check_embedded(core, ref, _corrupt(frag, [p]))
            row = (p % 8)
            assert code == (1 if row == 7 else 3), "a single error in bit %d" % p       # rows 0..6 are corrected, the parity row is only checked
            codes[code] += 1
    for trial in range(2000):
        lc9 = bytes(rng.randint(0, 256, 9).astype(np.uint8))
        frag = dmr_rx.matrix_fragments(dmr_rx.embedded_matrix(lc9))
        a, b = rng.choice(128, 2, replace=False)
        codes[_check_embedded(core, ref, _corrupt(frag, [int(a), int(b)]))] += 1
    for trial in range(300):            # heavier damage, so that miscorrections and checksum failures occur as well
        lc9 = bytes(rng.randint(0, 256, 9).astype(np.uint8))
        frag = dmr_rx.matrix_fragments(dmr_rx.embedded_matrix(lc9, crc=int(rng.randint(32)) if trial % 3 == 0 else None))
        pos = [int(p) for p in rng.choice(128, int(rng.randint(0, 5)), replace=False)]
        codes[_check_embedded(core, ref, _corrupt(frag, pos))] += 1
    assert all(codes.values()), codes


def test_python_matrix_is_the_reference_s(tx_ref):
    """the rule of dmr_rx.embedded_matrix, which builds the damaged fragments, against the fragments of the reference's encoder"""
    for lc9 in (dmr_rx.OWN, dmr_rx.PRIVATE, bytes(range(200, 209))):
        rec = np.stack([dmr_tx.record(dmr_tx.K_VOICE, fn=fn, cc=1, lc=lc9, payload=bytes(27)) for fn in (1, 2, 3, 4)])
        assert [dmr_rx.get_fragment(b) for b in tx_ref.bursts(rec)] == dmr_rx.matrix_fragments(dmr_rx.embedded_matrix(lc9))


def test_alias_buffer_bound(core):
    """The buffer is checked for completion after every append and cleared when complete; the header clears it first and brings 6 or 7 bytes;
    a block is appended only to an alias that is still incomplete and brings 7.  Incomplete means fewer than the need, and the largest need
    is format 3 with length 31: 62 bytes.  So the buffer holds at most 61 + 7 = 68 bytes, TA_MAX.  (With 7-byte blocks on a 6-byte header the
    sizes that occur are 6 + 7 k, so 62 is the most these streams reach: the format 3, length 31 alias completes exactly there.)"""
    assert dmr_rx.TA_MAX == 61 + 7 == core.lib.core_dmr_rx_sizes(3)
    assert core.lib.core_dmr_rx_sizes(0) == dmr_rx.REC and core.lib.core_dmr_rx_sizes(1) == dmr_rx.STATE_BYTES and core.lib.core_dmr_rx_sizes(2) == dmr_rx.STATE_PUBLIC
    most = {name: _run_core(core, name)[2] for name in NAMES}
    assert max(most.values()) <= dmr_rx.TA_MAX
    assert most["alias_format_3"] == 55       # held after a step; the next block completes it at 62
    _, _, want, _, _, _ = dmr_rx.scenario(G, "alias_format_3")
    done = want[(dmr_rx.flags(want) & dmr_rx.TALKER_ALIAS) != 0]
    assert [int(r[28]) for r in done] == [20, 62]


def test_alias_buffer_of_the_reference_never_exceeds_the_bound(ref):
    for name in ("alias_format_3", "alias_corners", "alias_formats_0_2"):
        _, inp, _, cc, prom, _ = dmr_rx.scenario(G, name)
        pending = []
        ref.run(inp, cc, prom, pending)
        assert max(pending) <= dmr_rx.TA_MAX and max(pending) > 0


def _flat_file(path):
    with open(path, "wb") as f:
        plain = dmr_rx.plain(G)
        f.write(struct.pack("<I", len(plain)))
        for k in plain:
            _, inp, want, cc, prom, _ = dmr_rx.scenario(G, NAMES[k])
            f.write(struct.pack("<Iii", inp.shape[0], cc, prom) + inp.tobytes() + want.tobytes())
    return len(plain), sum(int(G["counts"][k]) for k in plain)


def test_core_header_equals_the_golden_under_the_sanitizers(tmp_path):
    exe, data = str(tmp_path / "test_dmr_rx_core"), str(tmp_path / "golden.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_dmr_rx_core.cpp"), "-o", exe])
    s, n = _flat_file(data)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d scenarios, %d bursts" % (s, n)), r.stdout


# ------------------------------------------------------------------------------------------------------------------ the alias text on the host
FACADE = os.path.join(ROOT, "tests", "host", "test_dmr_rx_facade")


def _text(fmt, data):
    """dmr_alias_text of host/dmr_frame_hip.h through the facade's test driver, which needs no device for it"""
    if not os.path.exists(FACADE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "dmr_rx_facade"])
    r = subprocess.run([FACADE, "text", str(fmt), bytes(data).hex() or "-"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.strip()
    return b"" if out == "-" else bytes.fromhex(out)


def test_alias_text_of_the_golden_aliases():
    for name in ("whole_call", "alias_formats_0_2", "alias_format_3", "alias_corners"):
        _, _, want, _, _, _ = dmr_rx.scenario(G, name)
        for rec in want[(dmr_rx.flags(want) & dmr_rx.TALKER_ALIAS) != 0]:
            fmt, _, data = dmr_rx.alias_of(rec)
            text = _text(fmt, data)
            if fmt in (1, 2):
                assert text == data
            elif fmt == 3:
                assert text == data.decode("utf-16-be").encode()
            else:
                assert len(text) <= 8 * len(data) // 7 - 1 and text.isascii()      # the unpacking itself: the next test, against the reference's
    assert _text(3, "Hi😀".encode("utf-16-be")) == "Hi😀".encode() and _text(3, b"\xd8\x3d\x00A") == "�A".encode()
    assert _text(1, b"") == b"" and _text(0, b"") == b""


def test_alias_text_format_0_equals_the_reference_s_unpacking(tmp_path):
    if not os.path.isdir(os.path.join(dmr_rx.REFERENCE, "src", "DMR")):
        pytest.skip("the reference's sources are not here")
    import ctypes as C
    so = str(tmp_path / "libdmr_alias_ref.so")
    stub = os.path.join(ROOT, "tests", "host", "dmr_ctl_stub")
    subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-shared", "-fPIC"] + ["-D%s=dmr_alias_ref_%s" % (n, n) for n in ("QString", "QSysInfo", "DMRUtils")]
                          + [os.path.join(ROOT, "tests", "host", "dmr_alias_ref.cpp"), os.path.join(dmr_rx.REFERENCE, "src", "DMR", "dmrutils.cpp"),
                             "-I" + dmr_rx.REFERENCE, "-I" + dmr_rx.STUBS[0], "-I" + stub, "-o", so])
    lib = C.CDLL(so)
    rng = np.random.RandomState(5)
    for size in (7, 14, 21, 28, 8, 13, 1):
        data = bytes(rng.randint(0, 256, size).astype(np.uint8))
        out = bytearray(64)
        n = lib.ref_alias_7bit(data, size, dmr_tx.Ref.buf(out))
        want = bytes(out[1:n]).strip(b" \t\n\r\x0b\x0c")          # the reference drops the first character and trims
        want = "".join(chr(c) for c in want).encode()             # characters above 127 (the unpacking can make them) as UTF-8
        assert _text(0, data) == want, size
