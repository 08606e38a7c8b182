"""CPU: bench.py's command line, checked before anything touches the GPU."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True, timeout=300)


def test_steps_below_one_is_rejected():
    p = _bench("--steps", "0")
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, p.stderr[-2000:]


def test_help_lists_dump_outputs():
    p = _bench("--help")
    assert p.returncode == 0 and "--dump-outputs DIR" in p.stdout, p.stdout[-2000:]


def test_help_lists_full():
    p = _bench("--help")
    assert p.returncode == 0 and "--full" in p.stdout, p.stdout[-2000:]
