"""ctypes binding of libtvq_hip.so (include/tvq.h and include/tvq_fcn.h).

The library is loaded after `import torch` so that its NEEDED libamdhip64.so.7
resolves to the HIP runtime torch already mapped (same soname): the kernels
share torch's device context and streams.  There is no fallback: if the
library is missing or no GPU is present, the first call raises.

The headers are the single source of the signatures: SIGNATURES is parsed from include/tvq.h
and EXTRA_SIGNATURES from include/tvq_fcn.h at import (`parse_header`), and a declaration the
parser cannot map raises there.
"""
import ctypes
import os
import re
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get(
    "TVQ_HIP_LIB", os.path.join(os.path.dirname(os.path.dirname(_HERE)), "lib", "libtvq_hip.so"))

_lib = None
_lock = threading.Lock()

CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "csrc")
HEADER = os.path.join(CSRC, "..", "..", "include", "tvq.h")
FCN_HEADER = os.path.join(CSRC, "..", "..", "include", "tvq_fcn.h")


def source_hash():
    """The stamp csrc/Makefile compiles into the library (tvq_source_hash): sha1 of every
    csrc *.hip / *.h sorted by name, then include/tvq.h and include/tvq_fcn.h, first 16 hex
    digits."""
    import hashlib
    h = hashlib.sha1()
    names = sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".h")))
    for n in [os.path.join(CSRC, n) for n in names] + [HEADER, FCN_HEADER]:
        with open(n, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def built_hash(path=None):
    """tvq_source_hash() of the built library at `path` (None if missing or unstamped), read
    from the file's bytes (the literal "tvq_source_hash=<16 hex>" the Makefile compiles in):
    the library is not loaded, so a later ctypes.CDLL of a rebuilt file in this process is
    not handed a stale mapping, and the GPU is not initialised."""
    path = path or LIB_PATH
    if not os.path.exists(path):
        return None
    with open(path, "rb") as f:
        m = re.search(rb"tvq_source_hash=([0-9a-f]{16})", f.read())
    return m.group(1).decode() if m else None


_CTYPES = {  # every non-pointer type include/tvq.h may use; anything else raises
    "int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double,
    "tvq_stream_t": ctypes.c_void_p,
}
_PROTO = re.compile(r"((?:const\s+)?\w+[\s*]+)(tvq_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, named, where):
    """ctypes class of one C declaration: a parameter (`named`: its name follows the type)
    or a return type."""
    words = decl.replace("*", " * ").split()
    plain = re.fullmatch(r"[\w\s*]+", decl)  # no array, no function pointer
    if plain and "*" in words:  # char* is a C string, every other pointer an address
        base = [w for w in words[:words.index("*")] if w != "const"]
        return ctypes.c_char_p if base == ["char"] and words.count("*") == 1 else ctypes.c_void_p
    words = [w for w in words if w != "const"]
    if named and len(words) > 1:
        words = words[:-1]
    if not plain or len(words) != 1 or words[0] not in _CTYPES:
        raise ValueError(f"{where}: no ctypes mapping for '{decl.strip()}'")
    return _CTYPES[words[0]]


def parse_header(text, origin="tvq.h"):
    """name -> (argtypes, restype) of every `ret tvq_name(params);` in the header `text`.
    Raises on a type outside _CTYPES and on a `tvq_name(` that is no such prototype."""
    def blank(m):  # keeps the line numbers
        return re.sub(r"[^\n]", " ", m.group(0))

    text = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
    text = re.sub(r"^[ \t]*#[^\n]*", blank, text, flags=re.M)
    sigs, starts = {}, set()
    for m in _PROTO.finditer(text):
        ret, name, params = m.groups()
        where = f"{origin}:{text.count(chr(10), 0, m.start(2)) + 1}: {name}"
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = ([_ctype(p, True, where) for p in params], _ctype(ret, False, where))
        starts.add(m.start(2))
    for m in re.finditer(r"\btvq_\w+\s*\(", text):
        if m.start() not in starts:
            raise ValueError(f"{origin}:{text.count(chr(10), 0, m.start()) + 1}: "
                             f"'{m.group(0)}' is not a prototype this parser reads")
    return sigs


with open(HEADER) as _f:
    SIGNATURES = parse_header(_f.read(), HEADER)  # name -> (argtypes, restype)
with open(FCN_HEADER) as _f:  # the second public header; SIGNATURES stays tvq.h's table
    EXTRA_SIGNATURES = parse_header(_f.read(), FCN_HEADER)


class NativeError(RuntimeError):
    pass


def lib():
    """Load libtvq_hip.so once; raise loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"libtvq_hip.so not found at {LIB_PATH}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        h = ctypes.CDLL(LIB_PATH)
        for name, (args, res) in list(SIGNATURES.items()) + list(EXTRA_SIGNATURES.items()):
            fn = getattr(h, name)
            fn.argtypes = args
            fn.restype = res
        _lib = h
    return _lib


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Rejects CPU tensors loudly."""
    if t is None:
        return None
    if not t.is_cuda:
        raise NativeError("tvq HIP kernels need device tensors (got a CPU tensor); "
                          "the product path has no CPU fallback")
    return t.data_ptr()


POOL_SLOTS = 1 << 20
_pools = {}  # device index -> zeroed int32 counter pool registered with the library
_pool_dev = [-1]


def _ensure_pool(h):
    """Register this device's counter pool (tvq_counter_pool) on first use.  The first
    launch on a device is eager (warmup steps precede graph capture)."""
    dev = torch.cuda.current_device()
    if dev == _pool_dev[0]:
        return
    if dev not in _pools:
        pool = torch.zeros(POOL_SLOTS, dtype=torch.int32, device=dev)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize(dev)  # zeroed before any stream's kernel takes a slot
        rc = h.tvq_counter_pool(dev, pool.data_ptr(), POOL_SLOTS)
        if rc != 0:
            raise NativeError(f"tvq_counter_pool failed: {h.tvq_last_error().decode()}")
        _pools[dev] = pool
    _pool_dev[0] = dev


def call(name, *args):
    """Call an int-returning entry point; raise with tvq_last_error() on failure."""
    h = lib()
    _ensure_pool(h)
    rc = getattr(h, name)(*args)
    if rc != 0:
        raise NativeError(f"{name} failed ({rc}): {h.tvq_last_error().decode()}")
    return rc


def value(name, *args):
    return getattr(lib(), name)(*args)


class plan_trace:
    """Record the kernel variants the library's host-side plans launch (tvq_plan_trace);
    `.lines` holds them after the block (tests confirm which kernel a shape took)."""

    def __enter__(self):
        lib().tvq_plan_trace(1)
        self.lines = []
        return self

    def __exit__(self, *exc):
        h = lib()
        n = h.tvq_plan_read(None, 0)
        buf = ctypes.create_string_buffer(int(n) + 1)
        h.tvq_plan_read(buf, n + 1)
        h.tvq_plan_trace(0)
        self.lines = [s for s in buf.value.decode().split("\n") if s]
        return False

    def has(self, prefix):
        return [s for s in self.lines if s.startswith(prefix)]


def grad_sink(p):
    """p.grad when FusedAdamW keeps it as a view of its flat gradient buffer: backward
    kernels then accumulate straight into it and the autograd Function returns None
    for p (no AccumulateGrad kernel).  None otherwise (standard autograd return)."""
    if p is None or not getattr(p, "_tvq_flat", False) or not p.requires_grad:
        return None
    g = p.grad
    if g is None or not g.is_contiguous():
        return None
    return g


def grad_buffer(p, zeros=False):
    """(buf, direct) for a backward kernel that writes p's gradient: p's sink, which the
    kernel accumulates into (direct: pass accumulate = 1, return None for p), else a fresh
    tensor of p's shape to return (`zeros`: zero-filled, for a kernel that adds)."""
    sink = grad_sink(p)
    if sink is not None:
        return sink, True
    return (torch.zeros if zeros else torch.empty)(p.shape, device=p.device), False


def grad_buffers(params):
    """(grads, direct) for a backward kernel that writes several parameters' gradients under
    one accumulate flag (None entries: absent parameters, their gradient None).  All or
    nothing: the sinks when every present parameter has one (direct: return None for all),
    else fresh tensors of the parameters' shapes to return."""
    sinks = [grad_sink(p) for p in params]
    if all((s is not None) == (p is not None) for s, p in zip(sinks, params)):
        return sinks, True
    return [torch.empty(p.shape, device=p.device) if p is not None else None for p in params], False
