"""The REFERENCE's own tests of `MCMCSamples` and its integration scenario for the "emcee" and "minipcn" samplers, run unchanged
against this package (container only), exactly as tests/test_reference_unit_tests.py runs the rest: a child pytest on the file where
it lies under /root/reference, with tests/tools/ref_alias_plugin.py resolving `aspire.*` to this package.  With `MCMCSamples` in
`aspire_amd.samples` the plugin installs no placeholder for it, so the reference's tests build the real class.  The integration
cases additionally load tests/tools/mcmc_engine_plugin.py: the engine double with the recorder.  Skipped where /root/reference is
absent (the GPU box).
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
    # (file, -k selection, extra plugins, minimum number of tests that must run and pass)
    # from_chain, save / load of chain_shape, post_process (shared behaviour, no-op), __getitem__
    ("test_samples.py", "mcmc and not ptmcmc", (), 5),
    # test_integration_zuko: {None, float32, float64} x {emcee, minipcn} x {numpy, torch} x bounded_to_unbounded {True, False}
    ("integration_tests/test_integration.py", "not jax and not flowjax and (emcee or minipcn) and not smc", ("mcmc_engine_plugin",), 24),
]


@pytest.mark.parametrize("fname,select,plugins,at_least", CASES, ids=[os.path.basename(c[0]) for c in CASES])
def test_reference_mcmc_tests_pass_against_this_package(fname, select, plugins, at_least):
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests", "tools"), PYTHONDONTWRITEBYTECODE="1")
        cmd = [sys.executable, "-m", "pytest", os.path.join(REF_TESTS, fname), "-p", "ref_alias_plugin"]
        for p in plugins:
            cmd += ["-p", p]
        cmd += ["-o", "addopts=", "-p", "no:cacheprovider", f"--rootdir={tmp}", "-c", "/dev/null", "--import-mode=importlib", "-q",
                "-k", select, f"--confcutdir={os.path.dirname(REF_TESTS)}"]
        out = subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=900)
    tail = out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) >= at_least, tail
    last = out.stdout.splitlines()[-1]
    assert "failed" not in last and "skipped" not in last and "error" not in last, tail
