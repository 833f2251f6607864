#!/usr/bin/env python3
"""Run the device inflate's host twin (nerfhip_inflate_host) under AddressSanitizer and UndefinedBehaviorSanitizer, in a
stand-alone program, on a machine without a GPU.

    python tools/inflate_sanitize.py [--keep DIR]

Writes the whole corpus of tests/inflate_streams.py — zlib's streams, the hand-made accepted and refused ones, the truncated and
mutated ones — into one file, each with the verdict and the bytes recorded from zlib.decompress; compiles
tools/inflate_sanitize.cpp with csrc/inflate.hip (host code instrumented: -Xarch_host -fsanitize=address,undefined); runs it.  The
program inflates every stream alone and in batches, into heap blocks of exactly the documented sizes, and demands zlib's verdicts
and bytes; a sanitizer report ends it with a non-zero status.  Python is not in the instrumented process: nothing is preloaded."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
E_DATA = -4


def records():
    import inflate_streams
    for c in inflate_streams.corpus():
        name = c.name.encode()
        yield struct.pack("<4q", len(name), len(c.stream), c.out_bytes, 0 if c.expect is not None else E_DATA) + name + bytes(c.stream) \
            + (c.expect if c.expect is not None else b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="directory for the stream file and the program (default: a temporary one)")
    args = ap.parse_args()
    from nerf_pl_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        os.makedirs(work, exist_ok=True)
        cases = os.path.join(work, "inflate_cases.bin")
        with open(cases, "wb") as f:
            for r in records():
                f.write(r)
        exe = os.path.join(work, "inflate_sanitize")
        cmd = [build._hipcc(), "--offload-arch=" + build.ARCH, "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
               "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
               os.path.join(ROOT, "tools", "inflate_sanitize.cpp"), os.path.join(ROOT, "nerf_pl_amd", "csrc", "inflate.hip"),
               "-fsanitize=address,undefined", "-o", exe]
        subprocess.run(cmd, check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        return subprocess.run([exe, cases], env=env).returncode


if __name__ == "__main__":
    sys.exit(main())
