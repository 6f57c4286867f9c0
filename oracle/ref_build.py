"""Build recipe for oracle/_ref/libsift_ref.so: the reference's own
src/sift.cpp, compiled in place and unmodified over the stand-in OpenCV headers
of oracle/cvmini/, plus oracle/ref_wrap.cpp (extern "C" entry points).

TEST INFRASTRUCTURE ONLY.  The reference tree is named by SIFT_REFERENCE_DIR
(default /root/reference).  Where it does not exist this does nothing and
succeeds, and an existing oracle/_ref/ is left alone.  Nothing of the
reference is copied: the compiler reads it where it lies, and oracle/_ref/ is
ignored by git.

Flags: the reference makefile's line 25 (-std=c++11 -O3 -fopenmp) plus -fPIC;
no -march, no fast-math.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(HERE, "_ref")
LIB_PATH = os.path.join(REF_OUT, "libsift_ref.so")
CVMINI = os.path.join(HERE, "cvmini")
WRAP = os.path.join(HERE, "ref_wrap.cpp")
FLAGS = ["-std=c++11", "-O3", "-fopenmp", "-fPIC"]


def reference_dir() -> str:
    return os.environ.get("SIFT_REFERENCE_DIR", "/root/reference")


def reference_present() -> bool:
    return os.path.isfile(os.path.join(reference_dir(), "src", "sift.cpp"))


def _inputs():
    ref = reference_dir()
    files = [os.path.join(ref, "src", "sift.cpp"), os.path.join(ref, "include", "sift.hpp"), WRAP,
             os.path.abspath(__file__)]
    for d, _, names in os.walk(CVMINI):
        files += [os.path.join(d, n) for n in names]
    return files


def build(force: bool = False) -> str | None:
    """Returns the library's path, or None where there is no reference tree."""
    if not reference_present():
        return None
    if not force and os.path.exists(LIB_PATH):
        built = os.path.getmtime(LIB_PATH)
        if all(os.path.getmtime(f) <= built for f in _inputs()):
            return LIB_PATH
    ref = reference_dir()
    os.makedirs(REF_OUT, exist_ok=True)
    tmp = LIB_PATH + ".tmp"
    cmd = [os.environ.get("CXX", "g++")] + FLAGS + [
        "-I", CVMINI, "-I", os.path.join(ref, "include"), "-shared", "-o", tmp,
        os.path.join(ref, "src", "sift.cpp"), WRAP]
    subprocess.run(cmd, check=True)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    out = build(force="--force" in sys.argv)
    print(out if out else f"no reference tree at {reference_dir()}: nothing to build")
