"""numpy restatement of the random-push sampler (include/seqdex.h sdx_set_force_perturbation; csrc/sdx_randomize.hip
k_force_perturb), written from the definition, in float32 where the kernel is.  One call of `step` is one launch of the kernel for one
sdx_step / sdx_pre_physics.

  hash(seed ^ 0xF0CE, env * 256 + slot, step counter); slot 0: the push decision u' (first 24-bit uniform), slot 1: z_x, z_y (cos, sin of one
  Box-Muller pair), slot 2: z_z (cos), slot 3: the probability's u
  1 reset  rows of a resetting env <- 0, prob[e] <- exp((log lo - log hi) u + log hi)   (double, rounded once)
  2 decay  rows *= float32(decay ^ (dt / decay_interval))                                (double, rounded once)
  3 push   where u' < prob[e]: row of the target brick <- z * m * force_scale
"""
import numpy as np

from .noise_restatement import _fn, sdx_hash, uniforms

f32 = np.float32
TAG = 0xF0CE
BODIES, BODY_BRICK0 = 165, 32


def target_brick(env):
    """index of the env's target brick among the free bricks: env & 7 with {3, 4, 7} -> 0"""
    b = np.asarray(env) & 7
    return np.where((b == 3) | (b == 4) | (b == 7), 0, b)


def _hash(seed, n, slot, step):
    env = np.arange(n, dtype=np.uint64)
    return sdx_hash(seed ^ TAG, env * np.uint64(256) + np.uint64(slot), int(step))


def decay_factor(attr, dt):
    """decay^(dt / decay_interval) of the float32 inputs, in double, rounded once"""
    return f32(np.power(np.float64(f32(attr.decay)), np.float64(f32(dt)) / np.float64(f32(attr.decay_interval))))


def prob_draw(attr, seed, n, step):
    u, _ = uniforms(_hash(seed, n, 3, step))
    llo, lhi = np.log(np.float64(f32(attr.prob_lo))), np.log(np.float64(f32(attr.prob_hi)))
    return np.exp((llo - lhi) * u.astype(np.float64) + lhi).astype(f32)


def normals(seed, n, step):
    """[n, 3] standard normals of the push"""
    z = np.zeros((n, 3), f32)
    for slot, cols in ((1, (0, 1)), (2, (2,))):
        u0, u1 = uniforms(_hash(seed, n, slot, step))
        r, th = _fn(np.sqrt, f32(-2.0) * _fn(np.log, u0)), f32(6.28318530718) * u1
        z[:, cols[0]] = r * _fn(np.cos, th)
        if len(cols) == 2:
            z[:, cols[1]] = r * _fn(np.sin, th)
    return z


def step(attr, seed, step_count, rb_forces, prob, reset, mass, dt):
    """one launch: (rb_forces', prob', pushed [n] bool, z [n, 3]).  rb_forces [n, 165, 3] and prob [n] float32 as they are before the
    launch, reset [n] bool, mass [n] float32: the target brick's mass as the physics sees it."""
    n = prob.shape[0]
    F, p = np.array(rb_forces, f32), np.array(prob, f32)
    reset = np.asarray(reset, bool)
    F[reset] = 0
    p[reset] = prob_draw(attr, seed, n, step_count)[reset]
    F = (F * decay_factor(attr, dt)).astype(f32)
    u, _ = uniforms(_hash(seed, n, 0, step_count))
    pushed = u < p
    z = normals(seed, n, step_count)
    row = (z * np.asarray(mass, f32)[:, None]).astype(f32) * f32(attr.force_scale)
    body = BODY_BRICK0 + target_brick(np.arange(n))
    for e in np.nonzero(pushed)[0]:
        F[e, body[e]] = row[e]
    return F, p, pushed, z
