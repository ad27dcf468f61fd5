"""GPU tier: the spectral diffusion operator alone against fp64 on every kernel route of its dispatch, on the device -- condition-scaled error
under an a-priori bound and under 4 x torch's own fp32 error, the direct and wide routes proving that they ran -- and its contracts beyond
accuracy.  Bodies and criteria in diffusion_cases.py; every case leaves a ``diffusion_ops`` record in the margins file."""
import pytest

import diffusion_cases as dc
from test_head_gpu import dev  # noqa: F401  (the fixture binds the device build)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_diffusion(dev, case):
    dc.run_case(dev, case)


@pytest.mark.parametrize("case", dc.BASIS_CASES, ids=dc.case_id)
def test_basis_transforms(dev, case):
    dc.run_basis(dev, case)


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", list(dc.POISON_ROWS))
@pytest.mark.parametrize("K,C", dc.CONTRACT_WIDTHS)
def test_nonfinite_feature_stays_in_its_channel(dev, K, C, where, value):
    dc.run_nonfinite(dev, K, C, where, value)


@pytest.mark.parametrize("K,C", dc.CONTRACT_WIDTHS)
def test_nan_time_stays_in_its_channel(dev, K, C):
    dc.run_nonfinite(dev, K, C, "time", float("nan"))


@pytest.mark.parametrize("K,C", dc.CONTRACT_WIDTHS)
def test_underflow(dev, K, C):
    dc.run_underflow(dev, K, C)


@pytest.mark.parametrize("K,C", dc.CONTRACT_WIDTHS)
def test_determinism(dev, K, C):
    dc.run_determinism(dev, K, C)


@pytest.mark.parametrize("case", dc.WORKSPACE_CASES, ids=dc.case_id)
def test_exact_workspace(dev, case):
    dc.run_exact_workspace(dev, case)
