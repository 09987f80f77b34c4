"""CPU (-m "not gpu"): sim snapshots (include/seqdex.h sdx_state_*) on the EMULATED simulator - the product's
sdx_capi / task / physics / camera sources with csrc/sdx_state.h compiled by g++ for tests/hipemu.  The bodies are
tests/state_snapshot_cases.py; tests/test_gpu_state_snapshot.py runs them on the compiled gfx950 kernel.  Every comparison is exact."""
import pytest

torch = pytest.importorskip("torch")

import state_snapshot_cases as K          # noqa: E402
from tests.hipemu.sim import EmuSim       # noqa: E402

BACKEND = (lambda n, **kw: EmuSim(n, **kw), lambda t: t)
N = 26


@pytest.fixture(scope="module")
def sim26(golden_dir):
    s = K.make_scene_sim(BACKEND, golden_dir, N)
    yield s
    s.close()


def test_restore_all_brings_back_every_state_tensor_and_nothing_else(golden_dir):
    K.case_poison(BACKEND, golden_dir, N)


@pytest.mark.parametrize("resets", [False, True])
def test_replay_after_restore_all_is_bit_identical(golden_dir, resets):
    """resets=True: half the envs reset inside the window; the pile they draw is hash(seed, env, step_count), so the replay only matches
    when the step counter came back too"""
    K.case_replay(BACKEND, golden_dir, N, "grasp", resets=resets)


@pytest.mark.parametrize("use_clone", [False, True])
def test_restored_rows_and_clones_follow_their_source(golden_dir, use_clone):
    K.case_rows(BACKEND, golden_dir, N, use_clone)


@pytest.mark.parametrize("count", [0, 1, 7, N])
def test_row_lists_of_every_length(golden_dir, sim26, count):
    K.case_list_lengths(BACKEND, golden_dir, sim26, count)


def test_bad_entries_are_skipped_and_counted_and_bad_lists_refused(golden_dir):
    s = K.make_scene_sim(BACKEND, golden_dir, N, steps=1)
    try:
        K.case_skips(BACKEND, golden_dir, s)
    finally:
        s.close()


def test_warm_cache_counts_at_the_edges(sim26):
    """0, 1, 3, 4 (around one 16-byte piece), 1 535, 1 536 (the capacity) and an invalid 5 000 on envs 0 and 1, which is treated as 1 536"""
    K.case_warm_edges(BACKEND, sim26, [0, 1, 3, 4, 1535, 1536, 5000, -3])


def test_rows_travel_between_simulators_of_one_layout(golden_dir):
    K.case_across_handles(BACKEND, golden_dir, N, 10)


@pytest.mark.parametrize("kind,n", [("grasp", 8), ("orient", 4), ("insert", 6), ("search", 4)])
def test_replay_for_every_task_kind(golden_dir, kind, n):
    """Search's segmentation image and ten-frame buffer are part of the row (poisoned before the restore)"""
    K.case_replay(BACKEND, golden_dir, n, kind)


def test_insert_sim_classes_respect_env_mod_3(golden_dir):
    K.case_insert_classes(BACKEND, golden_dir, 25)


def test_replay_with_randomization_draws_the_same_samples(golden_dir):
    """randomization on, half the envs reset and are re-sampled inside the window: the DR_* rows and the draw counters come back, so the
    replay re-samples what the first run sampled"""
    K.case_replay(BACKEND, golden_dir, 8, "grasp", resets=True, randomize=True)
