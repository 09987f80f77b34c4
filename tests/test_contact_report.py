"""CPU (-m "not gpu"): the contact report and its reducer (include/seqdex.h sdx_set_contact_report / sdx_contact_wrenches, DESIGN.md
section 24) on the SIMT emulator: k_physics<512 | SDX_PHYS_REPORT ...>'s two write sites and k_contact_wrenches from their sources.

- the ABI: exports, the two struct mirrors, argument errors;
- armed changes nothing, bit for bit (randomization off / on, with and without a pending sdx_apply_dof_forces row); disarmed writes nothing;
- the report against the C oracle contact by contact; against SDX_T_CONTACT; Newton's second law on every free brick;
- the reducer against a float64 numpy reduction: a pile, an env in free flight, a rebuilt list.
The bodies are tests/contact_report_cases.py, shared with tests/test_gpu_contact_report.py."""
import ctypes as C

import pytest

from seqdex_amd import _abi

torch = pytest.importorskip("torch")

import contact_report_cases as K            # noqa: E402
from tests.hipemu.sim import EmuSim          # noqa: E402


class EmuReportSim(EmuSim):
    """the emulated simulator with the prototypes of the calls these tests make (tests/hipemu declares those of the calls it wraps itself)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        vp = C.c_void_p
        self.lib.sdx_set_contact_report.argtypes = [vp, C.POINTER(_abi.ContactReportStruct), vp]
        self.lib.sdx_contact_wrenches.argtypes = [vp, C.POINTER(_abi.ContactReportStruct), vp, C.POINTER(_abi.ContactPairs), vp, vp]
        self.lib.sdx_apply_dof_forces.argtypes = [vp, vp, C.c_uint32, vp]
        self.lib.sdx_set_randomization.argtypes = [vp, vp, vp]


BACKEND = (EmuReportSim, lambda t: t)


def test_abi_and_argument_errors():
    K.case_abi(BACKEND)


@pytest.mark.parametrize("randomize,dof_force", [(False, False), (True, False), (False, True), (True, True)])
def test_armed_changes_nothing(golden_dir, randomize, dof_force):
    K.case_armed_changes_nothing(BACKEND, golden_dir, randomize, dof_force)


def test_report_against_the_oracle(golden_dir):
    K.case_oracle_parity(BACKEND, golden_dir, "emulator")


def test_report_against_the_contact_tensor(golden_dir):
    K.case_contact_tensor(BACKEND, golden_dir)


def test_newton_on_the_bricks(golden_dir):
    K.case_newton(BACKEND, golden_dir, "emulator")


def test_reducer_against_numpy(golden_dir):
    K.case_reducer(BACKEND, golden_dir)
