"""bench.py's options that belong to a --full run are refused in a plain one (parsed before anything touches a GPU)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flag", ["--strong-leg", "--stream-leg"])
def test_legs_need_full(flag):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", flag, "on"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=ROOT)
    assert res.returncode == 2 and f"{flag} on needs --full" in res.stderr, res.stderr[-2000:]
    assert res.stdout == ""
