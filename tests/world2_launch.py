"""Start / wait / kill / collect for a pair of `tests/world2_rank.py` processes (world size 2 over gloo, file rendezvous).

Used by tests/test_world2_launcher.py (CPU-only scenarios: runs anywhere) and tests/test_gpu_world2.py (both ranks on the one
MI355X).  Each child runs under `timeout -k 10 <child_limit>` in a session of its own; the parent polls both, and the moment one
exits non-zero — or the parent's own limit passes — it kills both sessions and raises `World2Failure` with both stderr tails.
Nothing is retried and nothing is started after a failure."""
import os
import signal
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_PY = os.path.join(ROOT, "tests", "world2_rank.py")
WORLD = 2
KILL_AFTER = 10            # `timeout -k`: seconds between SIGTERM and SIGKILL at the child's limit


class World2Failure(RuntimeError):
    """A rank exited non-zero, or the pair outlived the parent's limit.  `.returncodes`, `.stderr` (per rank), `.pids` (the
    ranks' own process ids, as far as they got to write them), `.seconds`, `.partial` (what each rank saved before it failed)."""


def pid_alive(pid):
    """a process that exists and is not a zombie waiting to be reaped"""
    try:
        with open("/proc/%d/stat" % pid) as f:
            return f.read().rsplit(")", 1)[1].split()[0] not in ("Z", "X")
    except (OSError, IndexError):
        return False


def _tail(path, n=3000):
    try:
        with open(path, errors="replace") as f:
            return f.read()[-n:]
    except OSError:
        return ""


def _kill(procs):
    for p in procs:
        if p.poll() is None:
            try:
                os.killpg(p.pid, signal.SIGKILL)        # the `timeout` wrapper and the rank below it
            except ProcessLookupError:
                pass
    for p in procs:
        p.wait()


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True) if os.path.exists(path) else None


def run_pair(scenarios, workdir, child_limit=300, collective_timeout=120):
    """Run `scenarios` (names of world2_rank.SCENARIOS, in order) on two ranks.  Returns ([rank 0's results, rank 1's results],
    seconds): each `{scenario: {name: tensor | number | str | list}}`.  Raises World2Failure."""
    workdir = str(workdir)
    os.makedirs(workdir, exist_ok=True)
    tag = "pair%d_%d" % (os.getpid(), len(os.listdir(workdir)))
    rdzv, out = os.path.join(workdir, tag + ".rdzv"), os.path.join(workdir, tag)
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.setdefault("GLOO_SOCKET_IFNAME", "lo")          # both ranks are on this host
    procs, logs = [], []
    t0 = time.perf_counter()
    try:
        for r in range(WORLD):
            err = open("%s.rank%d.stderr" % (out, r), "w")
            logs.append(err)
            cmd = ["timeout", "-k", str(KILL_AFTER), str(child_limit), sys.executable, RANK_PY, str(r), str(WORLD), rdzv, out,
                   ",".join(scenarios), "--timeout", str(collective_timeout)]
            procs.append(subprocess.Popen(cmd, stdout=err, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, env=env, cwd=ROOT,
                                          start_new_session=True))
        deadline = t0 + child_limit + KILL_AFTER + 10     # the parent's own limit: past everything `timeout` does by itself
        why = None
        while why is None:
            codes = [p.poll() for p in procs]
            if any(c not in (None, 0) for c in codes):
                why = "exited non-zero"
            elif all(c == 0 for c in codes):
                break
            elif time.perf_counter() > deadline:
                why = "outlived the parent's limit of %d s" % (deadline - t0)
            else:
                try:
                    next(p for p in procs if p.poll() is None).wait(timeout=0.05)
                except subprocess.TimeoutExpired:
                    pass
        seconds = time.perf_counter() - t0
        if why is not None:
            first = [p.poll() for p in procs]             # as found: the rank that is still running shows None
            _kill(procs)
    finally:
        _kill(procs)
        for f in logs:
            f.close()
    paths = ["%s.rank%d" % (out, r) for r in range(WORLD)]
    if why is None:
        return [_load(p + ".pt") for p in paths], seconds
    pids = []
    for p in paths:
        try:
            pids.append(int(open(p + ".pid").read()))
        except (OSError, ValueError):
            pids.append(None)
    end = time.perf_counter() + 10
    while any(pid is not None and pid_alive(pid) for pid in pids) and time.perf_counter() < end:      # SIGKILL is not instantaneous
        time.sleep(0.01)
    lines = ["world-2 pair %s after %.1f s" % (why, seconds)]
    for r in range(WORLD):
        c = first[r]
        note = ("still running, killed" if c is None else "time limit of %d s: counts as a hang" % child_limit if c in (124, 137)
                else "exit status %d" % c)
        lines.append("---- rank %d (%s), end of its output:\n%s" % (r, note, _tail(paths[r] + ".stderr")))
    e = World2Failure("\n".join(lines))
    e.returncodes, e.pids, e.seconds = first, pids, seconds
    e.stderr = [_tail(p + ".stderr") for p in paths]
    e.partial = [_load(p + ".pt") for p in paths]
    raise e
