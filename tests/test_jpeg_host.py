"""CPU: tools/jpeg_host_check.cpp, built with -fsanitize=address,undefined by the host compiler, on every file of
tests/golden/jpeg_ingest.npz: the file, every truncation of it and every single-byte inversion must come back
from the C++ front end (csrc/jpeg_decode.h) with 0 or -1 and no read outside the input. A stand-alone program
with the sanitizer runtimes linked in: nothing is preloaded. Skipped when there is no host compiler (or it cannot link the sanitizer runtimes)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# the sanitizer runtimes linked into the program itself where the compiler can (GCC's flags; clang's default)
LINKS = (["-static-libasan", "-static-libubsan"], [])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    compilers = [cc for cc in ("g++", "c++", "clang++") if shutil.which(cc)]
    if not compilers:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("jpeg_host") / "jpeg_host_check")
    errors = []
    for cc in compilers:
        for link in LINKS:
            r = subprocess.run([cc] + FLAGS + link + ["-I", os.path.join(PKG, "csrc"),
                                                      os.path.join(ROOT, "tools", "jpeg_host_check.cpp"), "-o", exe],
                               capture_output=True, text=True)
            if r.returncode == 0:
                return exe
            errors.append(r.stderr)
    if all("san" in e for e in errors):
        pytest.skip("the host compiler cannot link the sanitizer runtimes")
    raise AssertionError(errors[0])


def test_front_end_is_clean_on_every_fixture_and_its_mutations(checker, golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "jpeg_ingest.npz"))
    names = [str(c) for c in g["cases"]] + [f"refuse_{r}" for r in g["refusals"]]
    files = []
    for n in names:
        files.append(str(tmp_path / f"{n}.jpg"))
        with open(files[-1], "wb") as f:
            f.write(g[f"{n}_jpg"].tobytes())
    r = subprocess.run([checker] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(names)
    for n, ln in zip(names, lines):
        assert ln.endswith("broken 0"), ln
        assert ("whole file refused" if n.startswith("refuse_") else "whole file decoded") in ln, ln
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
