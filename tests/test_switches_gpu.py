"""GPU tier: every off-default arm of the environment switches against the kernel references, on an MI355X.

tests/switch_cases.py holds the table and the child runner.  One test per set of arms; every set is a fresh child process started
with its environment by the launcher that was forked before this process touched the GPU (conftest.py: clean_launcher), one after
the other.  The children inherit the environment as found; the tests set no queue or device variable.

A child that ends by a signal, an abort or its time limit, or whose output reports an illegal memory access, has faulted the GPU
or hung on it: the module notes it and skips every set that has not run yet -- nothing is started on a card in that state, and
nothing is retried."""
import os
import subprocess
import sys

import pytest

import switch_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# hang guard per child, no performance claim: ten times the wall time of the baseline child on an MI355X, rounded up to 30 s, and
# at least 60 s
CHILD_TIMEOUT = 60   # the baseline child took 3.9 s on an MI355X (the other children 3.1 - 3.5 s): 10 x is below the 60 s floor
FAULT_CODES = (134, -6, 139, -11, 124, 137, -999)   # abort, segmentation fault, time limits; -999: the launcher's own timeout
FAULT_TEXT = "an illegal memory access was encountered"
_faulted = []


def _run(launcher, name):
    argv = [sys.executable, os.path.join(ROOT, "tests", "switch_cases.py"), "cuda:0", name]
    env = sc.child_env(name)
    if launcher is not None:
        return launcher.run(argv, env, CHILD_TIMEOUT)
    try:   # a single test run by hand without "-m gpu"
        r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        return -999, str(e.stdout or ""), repr(e)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("name", (sc.BASELINE,) + sc.SETS + (sc.ENGINE_SET,))
def test_switch_set_on_gpu(name, clean_launcher):
    if _faulted:
        pytest.skip(f"the child of set {_faulted[0]} faulted or hung on the GPU: no further child is started")
    rc, out, err = _run(clean_launcher, name)
    print(out[-8000:])
    if rc in FAULT_CODES or rc < 0 or FAULT_TEXT in out or FAULT_TEXT in err:
        _faulted.append(name)
    assert rc == 0 and f"switch set {name} ok" in out, f"return code {rc}\n" + out[-3000:] + err[-4000:]
