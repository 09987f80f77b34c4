"""CPU (-m "not gpu"): the pose solver (include/seqdex.h sdx_solve_ik) on the SIMT emulator: k_solve_ik compiled by g++.

- the ABI: the export, every argument error, the struct's size, version 8 and 56 tensor ids, the Python tensor checks;
- one step and eight steps of the law against the law in numpy float64;
- reach judged by refresh_kinematics(), the task masks, a start that is already there, unreachable targets;
- the limits under randomization, the call's independence of the step, N against 2 N.
The bodies are tests/ik_cases.py, shared with tests/test_gpu_ik.py."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

import ik_cases as K                         # noqa: E402
from seqdex_amd import _abi                  # noqa: E402
from tests.hipemu.sim import EmuSim          # noqa: E402


class EmuIkSim(EmuSim):
    """the emulated simulator with the prototype of the new call (tests/hipemu declares those of the calls it wraps itself)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        vp = C.c_void_p
        self.lib.sdx_solve_ik.argtypes = [vp, C.POINTER(_abi.IkAttr), vp, vp, vp, vp, vp, vp, vp, vp]


BACKEND = (EmuIkSim, lambda t: t)


def test_abi_exports_and_argument_errors():
    K.case_abi(BACKEND)


def test_one_step_of_the_law_against_float64():
    K.case_one_step(BACKEND)


def test_eight_steps_of_the_law_against_float64():
    K.case_fixed_loop(BACKEND)


def test_reach_judged_by_refresh_kinematics():
    K.case_reach(BACKEND)


def test_task_masks():
    K.case_masks(BACKEND)


def test_already_there():
    K.case_already_there(BACKEND)


def test_unreachable_targets():
    K.case_unreachable(BACKEND)


def test_limits_under_randomization():
    K.case_randomized_limits(BACKEND)


def test_independence_of_the_step():
    K.case_independence(BACKEND)


def test_first_n_rows_do_not_depend_on_n():
    K.case_n_against_2n(BACKEND)
