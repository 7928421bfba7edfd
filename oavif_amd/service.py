"""The resident scoring service (oavif_amd/csrc/oavif_scored.cpp) from Python.

    with service.start(max_lifetime=600) as svc:
        env = dict(os.environ, OAVIF_SCORER_SOCKET=svc.socket)      # for per-image child processes
        s = Ssimu2(0, service=svc.socket)                           # or a context of this process

One `oavif_scored` process owns the GPU; every process that creates its scorer context with OAVIF_SCORER_SOCKET set
talks to it and never starts HIP.  `python -m oavif_amd.service --socket PATH ...` runs one in the foreground.
"""
from __future__ import annotations

import argparse
import os
import select
import shutil
import signal
import subprocess
import sys
import tempfile
import time

from . import build as _build

ENV = "OAVIF_SCORER_SOCKET"


class ServiceError(RuntimeError):
    pass


class Service:
    """A running oavif_scored child: `.socket`, `.version` (its ssimu2_version()), `.stop()`; a context manager."""

    def __init__(self, proc: subprocess.Popen, socket: str, version: str, private_dir: str | None):
        self.proc, self.socket, self.version, self._dir = proc, socket, version, private_dir

    def stop(self, timeout: float = 10.0) -> int:
        """SIGTERM, wait, SIGKILL if it does not leave; returns the exit code (0 = orderly)."""
        if self.proc.poll() is None:
            self.proc.send_signal(signal.SIGTERM)
            try:
                self.proc.wait(timeout)
            except subprocess.TimeoutExpired:
                self.proc.kill()
                self.proc.wait()
        if self.proc.stdout:
            self.proc.stdout.close()
        if self._dir:
            shutil.rmtree(self._dir, ignore_errors=True)
            self._dir = None
        return self.proc.returncode

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.stop()


def command(socket: str, device: int = 0, idle_exit=None, max_lifetime=None, max_contexts=None, parent_pid=None,
            program: str | None = None) -> list:
    cmd = [program or _build.SERVICE_PATH, "--socket", socket, "--device", str(int(device))]
    for flag, v in (("--idle-exit", idle_exit), ("--max-lifetime", max_lifetime), ("--max-contexts", max_contexts),
                    ("--parent-pid", parent_pid)):
        if v is not None:
            cmd += [flag, str(v)]
    return cmd


def start(socket: str | None = None, device: int = 0, idle_exit=None, max_lifetime=None, max_contexts=None,
          ready_timeout: float = 60.0, program: str | None = None) -> Service:
    """Start the service as a fresh child process (never an exec of this one) and wait for its `ready` line.
    `socket` None: a socket in a new private directory (0700).  The child gets this process's environment unchanged
    (without OAVIF_SCORER_SOCKET: the service itself scores on the GPU) and --parent-pid, so it leaves with us.
    `program`: another build of the service (the CPU tests' one over a stand-in scorer)."""
    if program is None and _build.needs_build():
        _build.build()
    private = None
    if socket is None:
        private = tempfile.mkdtemp(prefix="oavif_scored_")   # mkdtemp: mode 0700
        socket = os.path.join(private, f"gpu{int(device)}.sock")
    env = {k: v for k, v in os.environ.items() if k != ENV}
    proc = subprocess.Popen(command(socket, device, idle_exit, max_lifetime, max_contexts, os.getpid(), program),
                            stdout=subprocess.PIPE, stdin=subprocess.DEVNULL, env=env)
    deadline = time.monotonic() + ready_timeout
    line = b""
    while not line.endswith(b"\n"):
        left = deadline - time.monotonic()
        if left <= 0 or not select.select([proc.stdout], [], [], left)[0]:
            break
        chunk = os.read(proc.stdout.fileno(), 4096)
        if not chunk:
            break
        line += chunk
    said, head = line.decode(errors="replace").rstrip("\n"), f"ready {socket} "
    if not said.startswith(head):
        proc.kill()
        rc = proc.wait()
        proc.stdout.close()
        if private:
            shutil.rmtree(private, ignore_errors=True)
        raise ServiceError(f"oavif_scored did not become ready within {ready_timeout:g} s (exit code {rc}, said {line!r})")
    return Service(proc, socket, said[len(head):], private)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m oavif_amd.service", description="run the scoring service in the foreground")
    ap.add_argument("--socket", required=True)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-contexts", type=int)
    ap.add_argument("--idle-exit", type=float)
    ap.add_argument("--max-lifetime", type=float)
    a = ap.parse_args(argv)
    svc = start(a.socket, a.device, a.idle_exit, a.max_lifetime, a.max_contexts)
    print(f"ready {svc.socket} {svc.version}", flush=True)
    signal.signal(signal.SIGTERM, lambda *_: svc.proc.send_signal(signal.SIGTERM))
    try:
        svc.proc.wait()
    except KeyboardInterrupt:
        pass
    return svc.stop()


if __name__ == "__main__":
    sys.exit(main())
