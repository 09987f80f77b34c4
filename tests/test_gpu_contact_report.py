"""-m gpu: the contact report and its reducer through the compiled gfx950 kernels: k_physics<516 .. 519> (the
SDX_PHYS_REPORT instantiations, alone and with SDX_PHYS_DR / SDX_PHYS_FORCE) and k_contact_wrenches.  The bodies are
tests/contact_report_cases.py, shared with the emulated run of tests/test_contact_report.py; the full-size case runs here only."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import contact_report_cases as K            # noqa: E402


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


BACKEND = (_make, lambda t: t.cuda())


def test_abi_and_argument_errors():
    K.case_abi(BACKEND)


@pytest.mark.parametrize("randomize,dof_force", [(False, False), (True, False), (False, True), (True, True)])
def test_armed_changes_nothing(golden_dir, randomize, dof_force):
    K.case_armed_changes_nothing(BACKEND, golden_dir, randomize, dof_force)


def test_report_against_the_oracle(golden_dir):
    K.case_oracle_parity(BACKEND, golden_dir, "MI355X")


def test_report_against_the_contact_tensor(golden_dir):
    K.case_contact_tensor(BACKEND, golden_dir)


def test_newton_on_the_bricks(golden_dir):
    K.case_newton(BACKEND, golden_dir, "MI355X")


def test_reducer_against_numpy(golden_dir):
    K.case_reducer(BACKEND, golden_dir)


def test_full_size_armed_against_unarmed():
    K.case_full_size(BACKEND)
