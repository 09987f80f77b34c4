"""-m gpu: sim snapshots (include/seqdex.h sdx_state_*) through the compiled gfx950 copy kernel, at N = 50 envs - the
smallest N with two envs in every class mod 24 (InsertSim's classes are env & 7 and env % 3).  The bodies are tests/state_snapshot_cases.py,
shared with the emulated run of tests/test_state_snapshot.py.  Every comparison is exact."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import state_snapshot_cases as K          # noqa: E402

N = 50


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


BACKEND = (_make, lambda t: t.cuda())


@pytest.fixture(scope="module")
def sim50(golden_dir):
    s = K.make_scene_sim(BACKEND, golden_dir, N)
    yield s
    s.close()


def test_restore_all_brings_back_every_state_tensor_and_nothing_else(golden_dir):
    K.case_poison(BACKEND, golden_dir, N)


@pytest.mark.parametrize("resets", [False, True])
def test_replay_after_restore_all_is_bit_identical(golden_dir, resets):
    K.case_replay(BACKEND, golden_dir, N, "grasp", resets=resets)


@pytest.mark.parametrize("use_clone", [False, True])
def test_restored_rows_and_clones_follow_their_source(golden_dir, use_clone):
    K.case_rows(BACKEND, golden_dir, N, use_clone)


@pytest.mark.parametrize("count", [0, 1, 7, N])
def test_row_lists_of_every_length(golden_dir, sim50, count):
    K.case_list_lengths(BACKEND, golden_dir, sim50, count)


def test_bad_entries_are_skipped_and_counted_and_bad_lists_refused(golden_dir):
    s = K.make_scene_sim(BACKEND, golden_dir, N, steps=1)
    try:
        K.case_skips(BACKEND, golden_dir, s)
    finally:
        s.close()


def test_warm_cache_counts_at_the_edges(sim50):
    K.case_warm_edges(BACKEND, sim50, [0, 1, 3, 4, 1535, 1536])      # (valid counts only)


def test_rows_travel_between_simulators_of_one_layout(golden_dir):
    K.case_across_handles(BACKEND, golden_dir, N, 10)


def test_insert_sim_classes_respect_env_mod_3(golden_dir):
    K.case_insert_classes(BACKEND, golden_dir, N)


def test_replay_with_randomization_draws_the_same_samples(golden_dir):
    K.case_replay(BACKEND, golden_dir, N, "grasp", resets=True, randomize=True)
