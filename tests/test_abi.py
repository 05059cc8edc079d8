"""The C-ABI library loads and exports every symbol include/tvq.h declares (CPU only)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tvq.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tvq_[A-Za-z0-9_]+)\s*\(", text)))


def test_header_declares_functions():
    names = declared_functions()
    assert "tvq_vq_assign" in names and "tvq_last_error" in names


def test_library_exports_every_declared_symbol():
    from timevqvae.hip import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail(f"{_native.LIB_PATH} missing: run __graft_entry__.build()")
    h = ctypes.CDLL(_native.LIB_PATH)
    missing = [n for n in declared_functions() if not hasattr(h, n)]
    assert not missing, missing
    h.tvq_abi_version.restype = ctypes.c_int
    assert h.tvq_abi_version() >= 1


def test_binding_covers_every_declared_symbol():
    from timevqvae.hip import _native
    missing = [n for n in declared_functions() if n not in _native.SIGNATURES]
    assert not missing, missing


def test_signatures_are_the_headers():
    """_native.SIGNATURES is parsed from the header: the same names as declared_functions()
    (185 today, the four tvq_convT2d_* among them), and one spot check per type rule."""
    from timevqvae.hip._native import SIGNATURES
    names = declared_functions()
    assert len(names) == 185 and "tvq_convT2d_fwd" in names
    assert sorted(SIGNATURES) == names
    args, res = SIGNATURES["tvq_vq_assign"]
    assert len(args) == 16 and res is ctypes.c_int
    assert args[10] is ctypes.c_int and args[9] is ctypes.c_int64  # int training, int64_t K
    assert args[0] is ctypes.c_void_p and args[-1] is ctypes.c_void_p  # const float*, the stream
    args, _ = SIGNATURES["tvq_vq_assign_svq"]
    assert args[14] is ctypes.c_uint64 and args[11] is ctypes.c_float  # offset, temp
    assert SIGNATURES["tvq_stat_kde"][0].count(ctypes.c_double) == 1
    assert SIGNATURES["tvq_source_hash"] == ([], ctypes.c_char_p)
    assert SIGNATURES["tvq_plan_read"] == ([ctypes.c_char_p, ctypes.c_int64], ctypes.c_int64)
    assert SIGNATURES["tvq_counter_pool"][0] == [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]


@pytest.mark.parametrize("text,word", [
    ("int tvq_a(int64_t n, long double x);", "long double x"),      # a type outside the table
    ("int tvq_a(unsigned n);", "unsigned"),
    ("long tvq_a(void);", "long"),                                   # ... as the return type
    ("int tvq_a(float v[3]);", "v[3]"),
    ("int tvq_a(int (*cb)(int));", "tvq_a("),                        # no plain prototype
    ("int tvq_ok(void);\n#define X 1\n/* c */ static inline int tvq_b(int a) { return a; }",
     ":3:"),                                                         # named by its line
])
def test_parser_rejects_what_it_cannot_map(text, word):
    from timevqvae.hip._native import parse_header
    with pytest.raises(ValueError) as e:
        parse_header(text)
    assert word in str(e.value), str(e.value)


def test_parser_reads_comments_and_preprocessor_lines_as_blank():
    from timevqvae.hip._native import parse_header
    text = "#define tvq_m(x) x\n/* int tvq_old(int a); */\n// tvq_gone(\nconst char* tvq_s(void);\n"
    assert parse_header(text) == {"tvq_s": ([], ctypes.c_char_p)}


def test_rng_draw():
    """rng.draw: off returns (None, 0) and leaves the per-step call index alone; on returns
    the device's seed tensor and one call_offset(site)."""
    import torch
    from timevqvae.hip import rng
    dev, site, calls = torch.device("cpu:0"), 5 << 40, rng._calls[0]
    try:
        rng.restart_calls()
        assert rng.draw(dev, site, on=False) == (None, 0) and rng._calls[0] == 0
        s1, o1 = rng.draw(dev, site)
        s2, o2 = rng.draw(dev, site, on=True)
        assert (o1, o2) == (site + 1, site + 2) and rng._calls[0] == 2
        assert s1 is s2 and s1 is rng.seed_tensor(dev)
    finally:
        rng._calls[0] = calls


def test_product_refuses_cpu_tensors():
    import torch
    from timevqvae.hip._native import NativeError, ptr
    with pytest.raises(NativeError):
        ptr(torch.zeros(3))


def test_library_stamp_matches_sources():
    """The library carries the hash of the sources it was built from (csrc/Makefile
    tvq_source_hash); __graft_entry__.build() rebuilds when it differs, so the library the
    GPU tests load is the tree's."""
    from timevqvae.hip import _native
    assert _native.built_hash() == _native.source_hash(), (
        f"libtvq_hip.so was built from other sources ({_native.built_hash()} vs "
        f"{_native.source_hash()}): run __graft_entry__.build()")


@pytest.mark.gpu
def test_mapped_library_is_the_trees(cuda):
    """On the GPU box: the libtvq_hip.so this process actually mapped (after a kernel ran
    through it) is the in-tree file, and its compiled-in stamp -- asked of the mapped library
    itself, not read from the file -- equals the hash of the sources in this tree."""
    import torch
    from timevqvae.hip import _native
    h = _native.lib()
    x = torch.zeros(64, device=cuda)
    _native.call("tvq_fill", _native.ptr(x), 64, 1.5, _native.stream_ptr())
    torch.cuda.synchronize()
    assert float(x.sum()) == 96.0
    mapped = sorted({ln.split()[-1] for ln in open("/proc/self/maps")
                     if ln.rstrip().endswith("libtvq_hip.so")})
    assert mapped == [os.path.realpath(_native.LIB_PATH)], mapped
    stamp = h.tvq_source_hash().decode()
    assert stamp == _native.source_hash(), f"mapped library {stamp} != sources {_native.source_hash()}"
    print(f"mapped {mapped[0]} stamp {stamp} extra '{h.tvq_build_extra().decode()}'")
