"""pytest plugin (container only; TEST INFRASTRUCTURE): loaded BEHIND ref_alias_plugin, it swaps the process-wide engine double for
the one with the stretch-move and chain-recorder entry points (tests/chain_ref.py), which the "emcee" and "minipcn" samplers need
and plain `OracleEngine` does not have.  ref_alias_plugin itself stays as it is.  Driven by tests/test_mcmc_reference_units.py.
"""
import ref_alias_plugin  # noqa: F401  (installs the aliases and puts tests/ on the path)

from aspire_amd import samples as samples_mod
from chain_ref import ChainOracleEngine

samples_mod._default_engine = ChainOracleEngine()
