"""CPU tier (emulator build of the same kernel sources): the spectral diffusion operator alone against fp64 on every kernel route of its
dispatch -- condition-scaled error under an a-priori bound and under 4 x torch's own fp32 error, on inputs that are hard on purpose -- and
its contracts beyond accuracy: non-finite values stay where torch keeps them, underflow, determinism, the exact workspace.  The case table
is checked against a restatement of the dispatch with no library at all.  Bodies and criteria in diffusion_cases.py."""
import pytest

import diffusion_cases as dc
from test_linear_emu import emu, needs_emulator  # noqa: F401  (the fixture binds the emulator build)


def test_case_table_reaches_every_route_and_both_sides_of_every_bound():
    dc.check_case_table()
    dc.check_case_table(n_cus=3)      # the emulator's workgroup count: the 13-mesh batch is refused there, the 3-mesh ones are direct


@needs_emulator
@pytest.mark.parametrize("case", [c for c in dc.CASES if c not in dc.EMU_SLOW_CASES], ids=dc.case_id)
def test_diffusion_on_emulator(emu, case):
    dc.run_case(emu, case)


@needs_emulator
@pytest.mark.parametrize("case", dc.BASIS_CASES, ids=dc.case_id)
def test_basis_transforms_on_emulator(emu, case):
    dc.run_basis(emu, case)


@needs_emulator
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", list(dc.POISON_ROWS))
@pytest.mark.parametrize("K,C", dc.CONTRACT_WIDTHS)
def test_nonfinite_feature_stays_in_its_channel_on_emulator(emu, K, C, where, value):
    dc.run_nonfinite(emu, K, C, where, value)


@needs_emulator
@pytest.mark.parametrize("K,C", dc.CONTRACT_WIDTHS)
def test_nan_time_stays_in_its_channel_on_emulator(emu, K, C):
    dc.run_nonfinite(emu, K, C, "time", float("nan"))


@needs_emulator
@pytest.mark.parametrize("K,C", dc.CONTRACT_WIDTHS)
def test_underflow_on_emulator(emu, K, C):
    dc.run_underflow(emu, K, C)


@needs_emulator
@pytest.mark.parametrize("K,C", dc.CONTRACT_WIDTHS)
def test_determinism_on_emulator(emu, K, C):
    dc.run_determinism(emu, K, C)


@needs_emulator
@pytest.mark.parametrize("case", dc.WORKSPACE_CASES, ids=dc.case_id)
def test_exact_workspace_on_emulator(emu, case):
    dc.run_exact_workspace(emu, case)
