"""The REFERENCE's own tests of `PTMCMCSamples`, run unchanged against this package, exactly as tests/test_mcmc_reference_units.py
runs those of `MCMCSamples`: a child pytest on tests/test_samples.py where it lies under /root/reference, with
tests/tools/ref_alias_plugin.py resolving `aspire.*` to this package.  With `PTMCMCSamples` in `aspire_amd.samples` the plugin installs
no placeholder for it, so the reference's tests build the real class.  Skipped where /root/reference is absent (the GPU box).
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

REF_TESTS = "/root/reference/tests"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not os.path.isdir(REF_TESTS), reason="the reference is only present in the build container")

# `-k ptmcmc` selects (case-insensitively) the nine test_ptmcmc_* functions - from_chain, __getitem__, four of subsample, thermodynamic
# integration against equations 35-37, two of the stepping-stone error - and the PTMCMCSamples case of the three tests parametrised
# over both chain containers (save / load, post_process, its no-op)
N_SELECTED = 12


def test_reference_ptmcmc_tests_pass_against_this_package():
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests", "tools"), PYTHONDONTWRITEBYTECODE="1")
        cmd = [sys.executable, "-m", "pytest", os.path.join(REF_TESTS, "test_samples.py"), "-p", "ref_alias_plugin", "-o", "addopts=",
               "-p", "no:cacheprovider", f"--rootdir={tmp}", "-c", "/dev/null", "--import-mode=importlib", "-q", "-k", "ptmcmc",
               f"--confcutdir={os.path.dirname(REF_TESTS)}"]
        out = subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=900)
    tail = out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == N_SELECTED, tail
    last = out.stdout.splitlines()[-1]
    assert "failed" not in last and "skipped" not in last and "error" not in last, tail
