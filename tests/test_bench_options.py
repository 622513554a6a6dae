"""bench.py's command line without a GPU: the options that only shape a --full run are refused in a plain one."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=240)


def test_repeats_needs_full():
    res = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--repeats", "2")
    assert res.returncode == 2 and "--repeats" in res.stderr and "--full" in res.stderr
    assert not res.stdout.strip()


def test_help_offers_full():
    res = _bench("--help")
    assert res.returncode == 0 and "--full" in res.stdout
