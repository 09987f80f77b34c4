"""CPU (-m "not gpu"): the restated streams of tests/helpers/device_rng.py are what they claim to be - the hash
against plain Python integers, the bit fields and constants, and the distribution of every draw at 4 sigma.  The GPU and emulator tests
(tests/test_gpu_act_noise.py, tests/reset_draw_cases.py, tests/test_gpu_tvalue_train.py) then only have to show device == restatement.

Every statistical condition is 4 standard errors of the quantity under the claimed distribution, for the sample stated in the test."""
import math

import numpy as np
import pytest

from helpers import device_rng as R
from helpers.noise_restatement import sdx_hash

f32 = np.float32
M64 = (1 << 64) - 1


def py_hash(seed, a, b):
    """csrc/sdx_common.h sdx_hash on Python integers"""
    z = (seed + 0x9E3779B97F4A7C15 * (a + 1) + 0xBF58476D1CE4E5B9 * (b + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ---------------------------------------------------------------------------------------------------------------- the hash, the fields
def test_hash_on_arrays_is_the_hash_on_integers():
    a = np.array([0, 1, 63, 64, 0xA11CE, 2 ** 40 + 7, M64], dtype=np.uint64)
    b = np.array([0, 1, 5, 1024 * 31 + 143, 2 ** 33, M64 - 1], dtype=np.uint64)
    for seed in (0, 22, 23, 5 ^ 0x5EED, M64):
        got = sdx_hash(seed, a[:, None], b[None, :])
        assert got.shape == (a.size, b.size) and got.dtype == np.uint64
        for i, ai in enumerate(a.tolist()):
            for j, bj in enumerate(b.tolist()):
                assert int(got[i, j]) == py_hash(seed, ai, bj), (seed, ai, bj)
        # Python integers in either place (the older callers pass b as an int, the act noise passes a as one)
        np.testing.assert_array_equal(sdx_hash(seed, a, 5), got[:, 2])
        np.testing.assert_array_equal(sdx_hash(seed, 63, b), got[2, :])


def test_act_noise_fields_and_constants():
    """u1 from bits 40..63 plus one, u2 from bits 8..31; the float32 factor of u1 is 2^-24 (16777217 is not a float32 number), so u1 reaches 1
    and the draw is then exactly zero - never a NaN or an infinity"""
    assert R.U1_SCALE == f32(2.0 ** -24) and R.U24 == f32(2.0 ** -24)
    eps, r, c, u1, u2 = R.act_noise_parts(22, 3, 5, 32)
    for e, col in ((0, 0), (4, 31), (2, 17)):
        h = py_hash(22, 3, e * 64 + col)
        assert float(u1[e, col]) == ((h >> 40) + 1) / 2.0 ** 24
        assert float(u2[e, col]) == ((h >> 8) & 0xFFFFFF) / 2.0 ** 24
        want_r = f32(math.sqrt(float(f32(-2.0) * f32(math.log(float(u1[e, col]))))))
        want_c = f32(math.cos(float(f32(6.28318530718) * u2[e, col])))
        assert r[e, col] == want_r and c[e, col] == want_c and eps[e, col] == want_r * want_c
    assert u1.min() >= f32(2.0 ** -24) and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    # the extreme fields: all ones (u1 = 1, the draw is 0) and all zeros (the largest radius)
    top = (np.array([0xFFFFFF, 0], dtype=np.float32) + f32(1.0)) * R.U1_SCALE
    assert top[0] == 1.0 and top[1] == f32(2.0 ** -24)
    assert math.sqrt(-2.0 * math.log(float(top[1]))) <= math.sqrt(2.0 * math.log(16777217.0))


def test_streams_do_not_depend_on_the_number_of_envs_and_columns():
    big = R.act_noise(22, 7, 64, 32)
    np.testing.assert_array_equal(R.act_noise(22, 7, 3, 23), big[:3, :23])
    np.testing.assert_array_equal(R.search_jitter(5, np.arange(4), 9), R.search_jitter(5, np.arange(32), 9)[:4])
    np.testing.assert_array_equal(R.pile_choice(5, [31, 2], 9, 7), R.pile_choice(5, np.arange(32), 9, 7)[[31, 2]])


def test_integer_draws_against_python_integers():
    envs = [0, 1, 7, 31, 1023]
    for step in (0, 1, 17):
        assert R.pile_choice(5, envs, step, 7).tolist() == [py_hash(5, e, step) % 7 for e in envs]
        assert R.insert_slot(5, envs, step, 5).tolist() == [py_hash(5 ^ 0x5EED, e, step) % 5 for e in envs]
        assert R.insert_slot(5, envs, step, 9000).tolist() == [py_hash(5 ^ 0x5EED, e, step) % 5000 for e in envs]      # range(0, 5000)
        assert R.insert_slot(5, envs, step, [1, 5, 5000, 5001, 3]).tolist() == [py_hash(5 ^ 0x5EED, e, step) % c for e, c in zip(envs, (1, 5, 5000, 5000, 3))]
        assert float(R.insert_yaw_half(5, step)) == float(f32(0.785)) * (py_hash(5, 0xA11CE, step) & 1)
        assert R.tv_rows(9, step, 412, 37, 6).tolist() == [py_hash(9, step, r) % (412 if r < 3 else 37) for r in range(6)]
        j = R.search_jitter(5, envs, step)
        assert j.shape == (5, 144) and j.dtype == np.float32
        for k, e in enumerate(envs):
            for i in (0, 1, 143):
                u = ((py_hash(5 ^ 0x5EA7, e * 1024 + i, step) >> 40) & 0xFFFFFF) / 2.0 ** 23 - 1.0
                assert j[k, i] == f32(u) * f32(0.02)
            u = ((py_hash(5 ^ 0x7A96, e, step) >> 40) & 0xFFFFFF) / 2.0 ** 23 - 1.0
            assert R.search_drop(5, envs, step)[k] == f32(u)
    yaws = {float(R.insert_yaw_half(5, s)) for s in range(1, 17)}
    assert yaws == {0.0, float(f32(0.785))}


def test_pile_choice_and_insert_yaw_share_the_untagged_seed():
    """both read sdx_hash(seed, ., step); the yaw's stream index 0xA11CE is env 0xA11CE's pile stream, so the two are
    distinct only while N <= 0xA11CE"""
    for step in range(1, 9):
        bit = int(R.pile_choice(5, [0xA11CE], step, 2)[0])
        assert float(R.insert_yaw_half(5, step)) == float(f32(0.785)) * bit


def test_tv_batch_rows_are_unit_vectors_near_their_dataset_rows():
    rng = np.random.default_rng(0)
    succ = rng.standard_normal((300, 4)).astype(f32)
    succ /= np.linalg.norm(succ, axis=1, keepdims=True)
    fail = rng.standard_normal((50, 4)).astype(f32)
    fail /= np.linalg.norm(fail, axis=1, keepdims=True)
    for it, B in ((0, 1024), (1, 6)):
        x = R.tv_batch(9, it, succ, fail, B)
        assert x.shape == (B, 4) and x.dtype == np.float32
        np.testing.assert_allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=2.0 ** -22)
        idx = R.tv_rows(9, it, 300, 50, B)
        src = np.where((np.arange(B) < B // 2)[:, None], succ[np.minimum(idx, 299)], fail[np.minimum(idx, 49)])
        # v = row + noise, |noise| <= 0.05 per component (0.1 in length), x = v / |v|: |x - v| <= 1.1 * 0.1 / 0.9 per component
        assert np.abs(x - src).max() < 0.05 + 0.11 / 0.9
    assert np.abs(R.tv_batch(9, 0, succ, fail, 6) - R.tv_batch(9, 1, succ, fail, 6)).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------- distributions
COUNTERS, ENVS, COLS = 16, 1024, 23


@pytest.fixture(scope="module")
def normal_streams():
    """seed -> [16 counters, 1024 envs, 23 columns] float64: seeds 22 and 23 are rank 0 and rank 1 of a shipped run"""
    return {s: np.stack([R.act_noise(s, c, ENVS, COLS) for c in range(COUNTERS)]).astype(np.float64) for s in (22, 23, 3)}


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("seed", [22, 23, 3])
def test_act_noise_is_standard_normal(normal_streams, seed):
    x = normal_streams[seed]
    n = x.size
    assert n == 376832
    mean, std = x.mean(), x.std()
    kurt = ((x - mean) ** 4).mean() / std ** 4
    tail = (np.abs(x) > 2.0).mean()
    lags = [_corr(x[:-1], x[1:]), _corr(x[:, :-1], x[:, 1:]), _corr(x[:, :, :-1], x[:, :, 1:])]
    print("seed %d: mean %.4f std-1 %.4f kurt-3 %.4f lags %s tail %.5f max %.3f" % (seed, mean, std - 1, kurt - 3, np.round(lags, 4).tolist(), tail, np.abs(x).max()))
    assert abs(mean) <= 4.0 / math.sqrt(n)
    assert abs(std - 1.0) <= 4.0 / math.sqrt(2.0 * n)
    assert abs(kurt - 3.0) <= 4.0 * math.sqrt(24.0 / n)
    for lag in lags:                                        # along the counter, the env and the column
        assert abs(lag) <= 4.0 / math.sqrt(n)
    p = math.erfc(2.0 / math.sqrt(2.0))                     # P(|z| > 2) = 0.0455
    assert abs(tail - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n)
    assert np.abs(x).max() <= math.sqrt(2.0 * math.log(16777217.0))
    assert np.abs(x).max() > 4.0                            # ... and the tail is there: n P(|z| > 4) = 24


def test_act_noise_of_two_ranks_is_uncorrelated(normal_streams):
    n = normal_streams[22].size
    assert abs(_corr(normal_streams[22], normal_streams[23])) <= 4.0 / math.sqrt(n)
    assert abs(_corr(normal_streams[22], normal_streams[3])) <= 4.0 / math.sqrt(n)


def _chi2(draws, k):
    cnt = np.bincount(draws.ravel(), minlength=k).astype(np.float64)
    assert cnt.size == k                                    # nothing outside [0, k)
    exp = draws.size / k
    return float(((cnt - exp) ** 2 / exp).sum())


@pytest.mark.parametrize("k", [4, 10, 50])
def test_pile_choice_is_uniform(k):
    d = np.stack([R.pile_choice(22, np.arange(4096), s, k) for s in range(1, 9)])
    dof = k - 1
    assert _chi2(d, k) <= dof + 4.0 * math.sqrt(2.0 * dof)


@pytest.mark.parametrize("cnt", [1, 5, 4999])
def test_insert_slot_is_uniform(cnt):
    d = np.stack([R.insert_slot(22, np.arange(4096), s, cnt) for s in range(1, 9)])
    dof = cnt - 1
    assert _chi2(d, cnt) <= dof + 4.0 * math.sqrt(2.0 * dof)
    # not the pile choice's stream: the two agree no more often than chance (1 / cnt, 4 sigma of a binomial)
    if cnt > 1:
        same = (d == np.stack([R.pile_choice(22, np.arange(4096), s, cnt) for s in range(1, 9)])).mean()
        assert abs(same - 1.0 / cnt) <= 4.0 * math.sqrt((1.0 / cnt) * (1.0 - 1.0 / cnt) / d.size)


def test_search_jitter_is_uniform_and_one_draw_per_coordinate():
    j = np.stack([R.search_jitter(22, np.arange(512), s) for s in range(1, 5)]).astype(np.float64)      # [4, 512, 144]
    n = j.size
    assert j.min() >= -0.02 and j.max() < 0.02 and j.min() < -0.0199 and j.max() > 0.0199
    sd = 0.02 / math.sqrt(3.0)
    assert abs(j.mean()) <= 4.0 * sd / math.sqrt(n)
    assert abs(j.std() - sd) <= 4.0 * sd * math.sqrt(0.8 / (4.0 * n))          # kurtosis 1.8: se(std) = sd sqrt((k - 1) / (4 n))
    x, y = j[:, :, 0::2], j[:, :, 1::2]
    assert abs(_corr(x, y)) <= 4.0 / math.sqrt(x.size)                         # x and y of a brick are two draws
    assert abs(_corr(j[:, :, :-2], j[:, :, 2:])) <= 4.0 / math.sqrt(n)         # neighbouring bricks
    assert abs(_corr(j[:-1], j[1:])) <= 4.0 / math.sqrt(n)                     # step to step
    assert abs(_corr(j[:, :-1], j[:, 1:])) <= 4.0 / math.sqrt(n)               # env to env


def test_search_drop_is_uniform_and_moves_x_and_y_together():
    envs = np.arange(4096)
    r = np.stack([R.search_drop(22, envs, s) for s in range(1, 9)]).astype(np.float64)
    n = r.size
    assert r.min() >= -1.0 and r.max() < 1.0 and r.min() < -0.999 and r.max() > 0.999
    sd = 1.0 / math.sqrt(3.0)
    assert abs(r.mean()) <= 4.0 * sd / math.sqrt(n)
    assert abs(r.std() - sd) <= 4.0 * sd * math.sqrt(0.8 / (4.0 * n))
    pos = R.search_drop_pos(22, envs, 3)
    assert pos.dtype == np.float32 and (pos[:, 2] == f32(0.9)).all()
    np.testing.assert_array_equal(pos[:, 0], f32(0.25) + r[2].astype(f32) * f32(0.2))
    np.testing.assert_array_equal(pos[:, 1], f32(0.19) + r[2].astype(f32) * f32(0.15))
    # not the jitter's stream
    assert abs(_corr(r[2, :512], R.search_jitter(22, np.arange(512), 3)[:, 0].astype(np.float64))) <= 4.0 / math.sqrt(512)
