"""The REFERENCE's own unit-test files, run unchanged against this package (container only).

tests/tools/ref_alias_plugin.py makes `aspire.samples`, `aspire.history`, `aspire.transforms`, `aspire.utils` resolve to this
package's modules; each case below runs one of the reference's test files where it lies under /root/reference in a child pytest and
requires every selected test to pass.  The selections name what is in scope (the containers and the composite /
flow transform either side of the SMC hot path); what they leave out is what section 2 leaves out: plotting, the MCMC /
parallel-tempering containers, the stand-alone per-stage transform classes (one device table here: DESIGN.md section 2), the jax
namespace (not installed).  Skipped where /root/reference is absent (the GPU box).
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

CASES = [
    # (file, -k selection, minimum number of tests that must run and pass)
    ("test_samples.py", "not jax and (basesamples or test_samples_ or smc or str_contains)", 29),
    ("test_history.py", "not jax and not plot and not smc_history_samples", 2),
    ("test_transforms.py", "not jax and (composite or flow_transform)", 30),
    # the end-to-end scenarios: fit -> sample_posterior with the importance and SMC samplers (both bounded settings, three dtypes, numpy and
    # torch inputs), save_config / save_flow, the likelihood hole with -inf / nan / +inf, auto_checkpoint / resume_from_file.  Left
    # out: the emcee / blackjax kernels and the stand-alone `minipcn` MCMC sampler, flowjax.
    ("integration_tests/test_integration.py", "not jax and not flowjax and not emcee and not blackjax and not (minipcn and not smc)", 46),
    ("integration_tests/test_checkpointing.py", "not jax", 20),
]


@pytest.mark.parametrize("fname,select,at_least", CASES, ids=[os.path.basename(c[0]) for c in CASES])
def test_reference_unit_tests_pass_against_this_package(fname, select, at_least):
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests", "tools"), PYTHONDONTWRITEBYTECODE="1")
        cmd = [sys.executable, "-m", "pytest", os.path.join(REF_TESTS, fname), "-p", "ref_alias_plugin", "-o", "addopts=",
               "-p", "no:cacheprovider", f"--rootdir={tmp}", "-c", "/dev/null", "--import-mode=importlib", "-q", "-k", select,
               # collection walks the test file's parent directories only up to here: an ordinary user may not list the ones above
               f"--confcutdir={os.path.dirname(REF_TESTS)}"]
        out = subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=900)
    tail = out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) >= at_least, tail
    assert "failed" not in out.stdout.splitlines()[-1], tail
