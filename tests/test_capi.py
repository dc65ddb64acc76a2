"""C-ABI checks that need no GPU: the library loads, exports every symbol the header
declares, and the ctypes signature table matches the header prototypes."""
import ctypes
import os
import re

import pytest

import pcms_amd  # noqa: F401  (registers the package)
from pcms_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcms_hip.h")


def _prototypes():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\bint\s+(pcms_\w+)\s*\(([^)]*)\)\s*;", src):
        protos[m.group(1)] = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
    return protos


def _code(arg: str) -> str:
    if arg == "hipStream_t s":
        return "s"
    if "*" in arg:
        return "p"
    t = arg.rsplit(" ", 1)[0].replace("const ", "").strip()
    return {"int": "i", "long": "l", "double": "d", "float": "f"}[t]


def test_header_matches_ctypes_table():
    protos = _prototypes()
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    for name, args in protos.items():
        assert "".join(_code(a) for a in args) == _lib.SIGNATURES[name], name


def test_library_loads_and_exports_every_symbol():
    lib = _lib.load()
    for name in _prototypes():
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name


def test_host_queries_without_gpu():
    assert _lib.query("pcms_conv3_chunk", _lib.BF16) == 32
    assert _lib.query("pcms_conv3_chunk", _lib.F32) == 8      # bf16x6: 8 fp32 channels per chunk
    assert _lib.query("pcms_conv3_chunk", _lib.F32X3) == 16
    # pack elements (activation dtype): bf16 32 per (chunk, tap, row); fp32 x6: 48 bf16 per
    # 8 channels = 24 floats; x3: 32 bf16 per 16 channels = 16 floats
    assert _lib.query("pcms_conv3_pack_elems", _lib.BF16, 64, 64) == 2 * 27 * 64 * 32
    assert _lib.query("pcms_conv3_pack_elems", _lib.F32, 64, 64) == 8 * 27 * 64 * 24
    assert _lib.query("pcms_conv3_pack_elems", _lib.F32X3, 64, 5) == 1 * 27 * 64 * 16
    assert _lib.query("pcms_conv3_mblocks", 2, 128, 128, 64) == 2 * 16 * 16 * 8
    assert _lib.query("pcms_loss_rows", 1 << 20) > 0


def test_stream_grid_cap_switch_caps_the_row_queries():
    """pcms_stream_grid_cap: v > 0 sets, v <= 0 queries, the old value is returned; the default
    leaves every row count at its own cap; it is part of the engine's allocation key."""
    assert "pcms_stream_grid_cap" in _lib.SWITCHES
    big = _lib.query("pcms_stream_grid_cap", -1)
    assert big >= 2 ** 30 and _lib.query("pcms_stream_grid_cap", 0) == big
    before = (_lib.query("pcms_loss_rows", 1 << 24), _lib.query("pcms_bn_bwd_rows", _lib.BF16, 64, 1 << 22),
              _lib.query("pcms_head_bn_bwd_rows", 1 << 20, 2))
    assert before == (1024, 512, 2048)
    try:
        assert _lib.query("pcms_stream_grid_cap", 3) == big
        assert _lib.query("pcms_stream_grid_cap", -1) == 3 and 3 in _lib.switches()
        assert (_lib.query("pcms_loss_rows", 1 << 24), _lib.query("pcms_bn_bwd_rows", _lib.BF16, 64, 1 << 22),
                _lib.query("pcms_head_bn_bwd_rows", 1 << 20, 2)) == (3, 3, 3)
        assert _lib.query("pcms_maxpool_bwd_bn_rows", _lib.F32, 2, 32, 32, 32, 64) == 3
        assert _lib.query("pcms_head_bwd_ws_floats", 1 << 20, 2, 2) == 4 * 2 * 65
        assert _lib.query("pcms_box_channel_sum_ws_floats", _lib.F32, 2, 64, 32, 32, 32) == 3 * 64
    finally:
        assert _lib.query("pcms_stream_grid_cap", big) == 3
    assert (_lib.query("pcms_loss_rows", 1 << 24), _lib.query("pcms_bn_bwd_rows", _lib.BF16, 64, 1 << 22),
            _lib.query("pcms_head_bn_bwd_rows", 1 << 20, 2)) == before
