"""include/tvq_fcn.h, the library's second public header: exported, bound through
_native.EXTRA_SIGNATURES (SIGNATURES stays include/tvq.h's table) and part of the source stamp
(CPU only)."""
import ctypes
import hashlib
import os
import re
import shutil

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tvq_fcn.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tvq_[A-Za-z0-9_]+)\s*\(", text)))


def test_header_declares_the_fcn_entry_points():
    names = declared_functions()
    assert {"tvq_fcn_conv_bn_relu", "tvq_fcn_head"} <= set(names)
    assert all(n.startswith("tvq_fcn_") for n in names), names


def test_library_exports_every_declared_symbol():
    from timevqvae.hip import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail(f"{_native.LIB_PATH} missing: run __graft_entry__.build()")
    h = ctypes.CDLL(_native.LIB_PATH)
    missing = [n for n in declared_functions() if not hasattr(h, n)]
    assert not missing, missing


def test_extra_signatures_are_the_headers_and_disjoint():
    from timevqvae.hip._native import EXTRA_SIGNATURES, SIGNATURES
    assert sorted(EXTRA_SIGNATURES) == declared_functions()
    assert not set(EXTRA_SIGNATURES) & set(SIGNATURES)
    args, res = EXTRA_SIGNATURES["tvq_fcn_conv_bn_relu"]
    assert res is ctypes.c_int and len(args) == 12
    assert args[:6] == [ctypes.c_void_p] * 6 and args[6:11] == [ctypes.c_int64] * 5
    assert args[11] is ctypes.c_void_p  # the stream
    assert EXTRA_SIGNATURES["tvq_fcn_packed_size"] == ([ctypes.c_int64] * 3, ctypes.c_int64)


def test_lib_applies_both_tables():
    from timevqvae.hip import _native
    h = _native.lib()
    assert h.tvq_fcn_conv_bn_relu.argtypes == _native.EXTRA_SIGNATURES["tvq_fcn_conv_bn_relu"][0]
    assert h.tvq_fcn_packed_size.restype is ctypes.c_int64
    assert h.tvq_fcn_packed_size(128, 6, 8) == 128 * 8 * 8  # Ci padded to the chunk of 8
    assert h.tvq_vq_assign.argtypes == _native.SIGNATURES["tvq_vq_assign"][0]


def test_source_hash_covers_the_fcn_header(tmp_path, monkeypatch):
    """source_hash() over a copy of the tree's sources equals the tree's and the hash taken
    by hand (csrc files by name, include/tvq.h, include/tvq_fcn.h); one more byte in the
    copy's tvq_fcn.h changes it."""
    from timevqvae.hip import _native
    want = _native.source_hash()
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    names = sorted(n for n in os.listdir(_native.CSRC) if n.endswith((".hip", ".h")))
    for n in names:
        shutil.copy(os.path.join(_native.CSRC, n), csrc / n)
    shutil.copy(_native.HEADER, tmp_path / "tvq.h")
    shutil.copy(_native.FCN_HEADER, tmp_path / "tvq_fcn.h")
    h = hashlib.sha1()
    for p in [csrc / n for n in names] + [tmp_path / "tvq.h", tmp_path / "tvq_fcn.h"]:
        h.update(p.read_bytes())
    assert h.hexdigest()[:16] == want
    monkeypatch.setattr(_native, "CSRC", str(csrc))
    monkeypatch.setattr(_native, "HEADER", str(tmp_path / "tvq.h"))
    monkeypatch.setattr(_native, "FCN_HEADER", str(tmp_path / "tvq_fcn.h"))
    assert _native.source_hash() == want
    with open(tmp_path / "tvq_fcn.h", "ab") as f:
        f.write(b"\n")
    assert _native.source_hash() != want
