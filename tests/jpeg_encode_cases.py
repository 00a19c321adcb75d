"""The cases of tests/golden/jpeg_encode.npz for the encoder tests, and the restatement's file of each, computed once
per process and shared."""
import functools
import os

import numpy as np

import jpeg_encode_ref as ref

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode.npz"))
GROUPS = [str(g) for g in GOLD["groups"]]
SAMPLING = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}


def group(name):
    """`<W>x<H>_<sampling>_q<q>` -> (size key, sampling as the API spells it, quality, [contents])."""
    size, s, q = name.split("_")
    return size, SAMPLING[s], int(q[1:]), [str(c) for c in GOLD[f"contents_{size}"]]


def source(size, kind):
    return GOLD[f"src_{size}_{kind}"]


def golden(name, kind, what):
    """what: "coef" or "pix" of PIL's file for this group and content."""
    size, s, q = name.split("_")
    return GOLD[f"{size}_{kind}_{s}_{q}_{what}"]


@functools.lru_cache(maxsize=None)
def ref_file(name, kind):
    size, sampling, quality, _ = group(name)
    return ref.encode(source(size, kind), quality, sampling)
