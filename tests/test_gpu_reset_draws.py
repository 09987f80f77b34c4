"""-m gpu: the draws a reset makes for itself - pile choice, InsertSim's plate yaw and harvest-ring slot, Search's
lattice jitter and target drop - through the compiled gfx950 k_pre_physics, against the numpy restatement of
tests/helpers/device_rng.py.  The bodies are tests/reset_draw_cases.py, shared with the emulated run of tests/test_reset_draws.py.
No case passes a pile choice: the device's own draw is what is checked."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import reset_draw_cases as K          # noqa: E402


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


BACKEND = (_make, lambda t: t.cuda())


@pytest.mark.parametrize("kind", ["grasp", "orient", "insert", "search"])
def test_pile_choice(kind):
    K.case_pile_choice(BACKEND, kind)


def test_insert_slot_and_plate_yaw():
    K.case_insert(BACKEND)


def test_search_jitter_and_target_drop():
    K.case_search(BACKEND)
