"""The 16-bit per-pair path record (wh_set_path_buffer16), host side: what the header declares, what the built library
exports, and the argument check - no GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "witch_hip.h")
LIB = os.path.join(ROOT, "witch_amd", "libwitch_hip.so")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_entry_point_and_the_two_band_bits():
    h = _header()
    assert re.search(r"\bint\s+wh_set_path_buffer16\s*\(\s*wh_ehmm\s*\*\s*\w+\s*,\s*uint16_t\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+wh_set_path_buffer\s*\(\s*wh_ehmm\s*\*\s*\w+\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;", h)     # the 8-bit one stays
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(WH_PATH_\w+)\s+(\d+)", h)}
    assert consts["WH_PATH_BAND_KEPT"] == 256 and consts["WH_PATH_BAND_FAIL"] == 512
    # the low byte is what it was
    assert [consts[n] for n in ("WH_PATH_P2_WIN", "WH_PATH_P2_FULL", "WH_PATH_P4_W256", "WH_PATH_P4_W512", "WH_PATH_P4_WFAIL",
                                "WH_PATH_P4_FULL", "WH_PATH_DENSE", "WH_PATH_MULTI")] == [1, 2, 4, 8, 16, 32, 64, 128]
    vals = sorted(consts.values())
    assert len(set(vals)) == len(vals) and sum(vals) == 1023


def test_library_exports_the_symbol_and_refuses_a_null_handle():
    if not os.path.exists(LIB):
        pytest.skip("libwitch_hip.so is not built")
    lib = C.CDLL(LIB)
    fn = lib.wh_set_path_buffer16
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p]
    einval = int(re.search(r"#define\s+WH_EINVAL\s+\(?(-?\d+)\)?", _header()).group(1))
    assert einval != 0
    assert fn(None, None) == einval
    buf = (C.c_uint16 * 4)()
    assert fn(None, C.addressof(buf)) == einval
