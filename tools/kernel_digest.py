#!/usr/bin/env python3
"""Registers, scratch, LDS, occupancy, code size and an instruction-stream hash of every gfx950 kernel of libnerfhip.  No GPU needed.

    python tools/kernel_digest.py > new.txt                      # every compile job of nerf_pl_amd.build
    python tools/kernel_digest.py mlp_bwd_chain mlp_dx           # only the jobs whose object name starts with one of these
    python tools/kernel_digest.py png gif                        # e.g. the PNG encoder's kernels beside the GIF's
    python tools/kernel_digest.py inflate                        # the device inflate's one kernel
    python tools/kernel_digest.py jpeg                           # jpeg.hip's two kernels and jpeg_entropy.hip's seven
    python tools/kernel_digest.py baked                          # the baked-volume build and march kernels
    python tools/kernel_digest.py meshcast                       # the mesh hierarchy's build, the cast, shade and compose
    python tools/kernel_digest.py decimate                       # the mesh decimation's kernels
    python tools/kernel_digest.py texture                        # the texture atlas' points, gather and lookup
    python tools/kernel_digest.py --against old.txt > both.txt   # side by side with an earlier output, differences marked

The jobs are nerf_pl_amd.build._jobs() — the same sources, flags and per-file -mllvm options as the library build (with
NERFHIP_EXTRA_FLAGS and the NERFHIP_*_SCHED variables applied the same way) — compiled with `--cuda-device-only -S`.  The hash covers
the lines between a kernel's label and its .Lfunc_end with comments and directives dropped and local labels renumbered in order of
first appearance: two builds with equal hashes run the same instructions, whichever translation unit the kernel was compiled in.
"""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_pl_amd import build as nbuild  # noqa: E402

FIELDS = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"), ("lds", "LDSByteSize"),
          ("occ", "Occupancy"), ("code", "codeLenInByte"))
_LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def stream_hash(lines):
    """sha256 (first 16 hex digits) of the instructions: comments and directives dropped, local labels renumbered."""
    names = {}
    h = hashlib.sha256()
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if not line or (line.startswith(".") and not _LOCAL.match(line)):
            continue
        h.update(_LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line).encode() + b"\n")
    return h.hexdigest()[:16]


def kernels_of(asm):
    """{mangled name: {field: value, 'hash': ...}} of one device assembly listing"""
    lines = asm.splitlines()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        rec = {"hash": stream_hash(lines[start + 1:end])}
        for line in lines[end:]:                       # the resource comments follow the function; the next label ends them
            m = re.match(r";\s*(\w+)\s*[:=]\s*(\d+)", line)
            if m:
                rec.setdefault(m.group(1), m.group(2))
            elif re.match(r"[^\s;.]\S*:", line):
                break
        out[name] = rec
    return out


def digest_job(job):
    src, obj, flags = job
    unit = os.path.basename(obj)[:-2]
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, unit + ".s")
        r = subprocess.run([nbuild._hipcc()] + flags + ["--cuda-device-only", "-S", src, "-o", s], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (unit, r.stderr))
        with open(s) as fh:
            return unit, kernels_of(fh.read())


def read_table(path):
    """{mangled name: [columns]} of an earlier output"""
    with open(path) as fh:
        return {c[0]: c[1:] for c in (line.split() for line in fh if line.strip() and not line.startswith("#"))}


def main(argv):
    against = None
    if "--against" in argv:
        i = argv.index("--against")
        against = read_table(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    jobs = [j for j in nbuild._jobs() if not argv or any(os.path.basename(j[1]).startswith(a) for a in argv)]
    rows = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(os.cpu_count() or 4, 16, len(jobs) or 1))) as ex:
        for unit, kernels in ex.map(digest_job, jobs):
            for name, rec in kernels.items():
                rows[name] = [rec.get(key, "?") for _, key in FIELDS] + [rec["hash"], unit]
    print("# kernel  " + "  ".join(f for f, _ in FIELDS) + "  hash  unit" + ("  |  the same of --against  |  verdict" if against is not None else ""))
    bad = 0
    for name in sorted(set(rows) | set(against or {})):
        new, old = rows.get(name), (against or {}).get(name)
        line = name + "  " + "  ".join(new or ["-"])
        if against is not None:
            if new is None and argv:                   # (a subset was asked for: kernels of other units are not missing)
                continue
            verdict = "MISSING" if new is None else "NEW" if old is None else "same" if new[:-1] == old[:-1] else \
                      "resources-same-hash-differs" if new[:-2] == old[:-2] else "DIFFERS"
            bad += verdict not in ("same", "resources-same-hash-differs")
            line += "  |  " + "  ".join(old or ["-"]) + "  |  " + verdict
        print(line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
