"""The seeded sweep of tests/tools/csr_kernel_sweep.py on the device, one test per leg: every kernel that consumes the rating CSR
under the rules of rk_knn_norms, chained as its driver chains it, on generated cases with every parameter drawn at once, each
output against its numpy restatement and against the relations the header states (band, order, user_block and launch form change
no bit; a pair score is the matrix entry; the UserKNN tables' kept weights are DegSim's topw), exactly, behind sentinel guards.
The case counts are the ones the host side was timed with (the tool's docstring); tests/test_csr_kernel_sweep_host.py shows over
the same cases what the sweep reaches and which wrong kernels it would see.  A failure names (seed, index): case(seed, index)
of the tool rebuilds the case."""
import pytest

from tests.test_csr_kernel_sweep_host import patch_one_rule
from tests.tools import csr_kernel_sweep as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("leg,n_cases", [("neighbours", 200), ("rp3", 120), ("catchsync", 400)])
def test_sweep(gpu_device, leg, n_cases):
    assert n_cases == S.N_CASES[leg], "the count the host time was measured with"
    S.run(S.SEED, n_cases, leg, gpu_device)


@pytest.mark.parametrize("leg,entry", [("neighbours", "rk_itemknn_scores"), ("rp3", "hand-made parts"), ("catchsync", "rk_cs_cells")])
def test_sweep_reports_a_wrong_expectation(gpu_device, monkeypatch, leg, entry):
    """The device side of the comparison is live: with one rule of the restatements changed (a fused multiply-add in the ItemKNN
    score, the RP3beta weight multiplied in another order, the CatchSync bucket one bit lower) the pass stops within 40 cases at
    the entry that rule feeds, and the report carries what rebuilds the case."""
    patch_one_rule(leg, monkeypatch)
    with pytest.raises(S.Mismatch, match=entry) as err:
        S.run(S.SEED, 40, leg, gpu_device)
    report = str(err.value)
    assert f"rebuild with case({S.SEED}, " in report and "elements differ, first at [[" in report and "'k': " in report
