#!/usr/bin/env python3
"""Run the split entropy decoder's host twin (nerfhip_jpeg_entropy_decode_split) under AddressSanitizer and
UndefinedBehaviorSanitizer, in a stand-alone program, on a machine without a GPU.

    python tools/jpeg_split_sanitize.py [--keep DIR]

Writes the streams of tests/tools/jpeg_synth.py (edge and damaged ones), the baseline files of tests/golden/jpeg_mini, their
truncations and scans with random bytes changed into one file; compiles tools/jpeg_split_sanitize.cpp with csrc/jpeg.hip and
csrc/jpeg_entropy.hip (host code instrumented: -Xarch_host -fsanitize=address,undefined); runs it.  The program decodes every
stream sequentially and split at 32, 64, 256, 1024 and 4096 bits and demands equal verdicts and coefficients; a sanitizer report
ends it with a non-zero status.  Python is not in the instrumented process: nothing is preloaded."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
E_DATA = -4


def record(name, parsed, verdict):
    comps = parsed["components"]
    comp = [v for c in comps for v in (c[1], c[2], c[4], c[5])] + [0] * (12 - 4 * len(comps))
    table = np.zeros((8, 272), np.uint8)
    mask = 0
    for (tc, th), (counts, symbols) in parsed["huffman"].items():
        table[4 * tc + th, :16] = counts
        table[4 * tc + th, 16:16 + len(symbols)] = symbols
        mask |= 1 << (4 * tc + th)
    name = name.encode()
    scan = bytes(parsed["scan"])
    head = [len(name), len(comps)] + comp + [parsed["mcus_x"], parsed["mcus_y"], parsed["restart_interval"], mask, len(scan), verdict]
    return struct.pack("<20i", *head) + name + table.tobytes() + scan


def streams():
    import jpeg_synth
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.imageio_min import jpeg_parse

    def verdict(parsed):
        try:
            ops.jpeg_entropy_decode(parsed)
            return 0
        except NerfHipError:
            return E_DATA
    jpegs = os.path.join(ROOT, "tests", "golden", "jpeg_mini")
    standard = jpeg_parse(os.path.join(jpegs, "q90_420_61x45.jpg"))["huffman"]
    out = [record(n, p, 0) for n, p, _ in jpeg_synth.edge_cases(standard)]
    out += [record(n, p, E_DATA) for n, p in jpeg_synth.damaged_cases(standard)]
    rng = np.random.default_rng(5)
    for f in sorted(os.listdir(jpegs)):
        if not f.endswith(".jpg") or "progressive" in f:
            continue
        parsed = jpeg_parse(os.path.join(jpegs, f))
        out.append(record(f, parsed, 0))
        scan = parsed["scan"]
        for cut in (1, len(scan) // 3, len(scan) - 1):
            if cut >= 1:
                p = dict(parsed, scan=scan[:cut])
                out.append(record("%s cut at %d" % (f, cut), p, verdict(p)))
        for i in range(4):
            changed = bytearray(scan)
            for _ in range(3):
                changed[int(rng.integers(0, len(changed)))] = int(rng.choice([0xff, 0x00, 0xd0, 0xd9, int(rng.integers(0, 256))]))
            p = dict(parsed, scan=bytes(changed))
            out.append(record("%s noise %d" % (f, i), p, verdict(p)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="directory for the stream file and the program (default: a temporary one)")
    args = ap.parse_args()
    from nerf_pl_amd import build
    build.build(verbose=False)
    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        os.makedirs(work, exist_ok=True)
        cases = os.path.join(work, "jpeg_split_cases.bin")
        with open(cases, "wb") as f:
            f.write(b"".join(streams()))
        exe = os.path.join(work, "jpeg_split_sanitize")
        csrc = os.path.join(ROOT, "nerf_pl_amd", "csrc")
        cmd = [build._hipcc(), "--offload-arch=" + build.ARCH, "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
               "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
               os.path.join(ROOT, "tools", "jpeg_split_sanitize.cpp"), os.path.join(csrc, "jpeg.hip"),
               os.path.join(csrc, "jpeg_entropy.hip"), "-fsanitize=address,undefined", "-o", exe]
        subprocess.run(cmd, check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        return subprocess.run([exe, cases], env=env).returncode


if __name__ == "__main__":
    sys.exit(main())
