"""The ctypes table of the binding (timevqvae.hip._native.SIGNATURES), one line per entry point,
sorted: name, restype, argtypes by ctypes class name.  Needs no GPU and no library, so two
checkouts' tables compare with `diff`.

usage: python tools/abi_table.py [--root TREE]"""
import argparse
import os
import sys

ap = argparse.ArgumentParser(usage=__doc__)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ap.parse_args().root, "t-vq-vae-trajgen_amd"))
from timevqvae.hip import _native  # noqa: E402

for name, (args, res) in sorted(_native.SIGNATURES.items()):
    print(name, res.__name__, *(a.__name__ for a in args))
