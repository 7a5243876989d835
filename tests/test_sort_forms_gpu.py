"""The depth sort's non-default forms (csrc/depth_sort.hip): SGS_DS_CHAIN=0 -- rounds 2-5's passes behind three counting kernels, the
form every sort past 64 groups takes -- at 16, 8 and 4 waves per workgroup (SGS_DS_WAVES).  Both variables are read once per process,
so each form runs in a fresh child process (tests/sort_forms_child.py), one after the other."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sort_forms_child.py")


@pytest.mark.parametrize("waves", [16, 8, 4])
def test_unchained_sort_form_in_a_fresh_process(waves):
    """Bare keys (1 000 003 / 5 000 000 / 8 388 609 keys, random and depth-like with 10 % culled) against the stable sort, and a
    300 000-Gaussian forward against the oracle followed by a deferred forward with the same count and image."""
    env = dict(os.environ, SGS_DS_CHAIN="0", SGS_DS_WAVES=str(waves))
    r = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exited with {r.returncode}\n--- stderr ---\n{r.stderr[-6000:]}\n--- stdout ---\n{r.stdout[-2000:]}"
    assert f"SGS_DS_WAVES={waves}: ok" in r.stdout
