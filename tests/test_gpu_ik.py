"""-m gpu: the pose solver through the compiled gfx950 kernel k_solve_ik.  The bodies are tests/ik_cases.py, shared
with the emulated run of tests/test_ik.py; N = 3 (one env per workgroup: no pack size to straddle), and N against 2 N."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ik_cases as K                         # noqa: E402


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


BACKEND = (_make, lambda t: t.cuda())


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
