"""contact-by-contact comparison of a warm-start cache of the kernel (device or emulated source) with the C oracle's (test infrastructure:
uses the oracle).  A cache holds, per env, the identity keys and impulses of the contacts of the step's last solve; decoded with
tests/helpers/contact_keys.py the two sides' identities are comparable tuples
((kind, index) of body a, (kind, index) of body b, box pair, direction, sample), and bits 28..31 of a key are the contact's age (the
number of consecutive solves it has existed before this one, saturating at 15), which scales the warm start.

boundary_pairs() names, from the oracle alone, the box pairs in which two correct implementations may list different samples: those with a
sample so close to the inclusion threshold that the rounding of its coordinates decides on which side it falls."""
import numpy as np

from oracle import physics_oracle as po
from tests.helpers.contact_keys import decode_kernel, decode_oracle

# m, twice the 1 um tie margin of the collision rule (MANIFOLD_TIE_L): from bit-identical start states the compiled kernel and the oracle
# differ only by fma contraction on coordinates of about 1 m magnitude (2^-24 relative per operation, a few operations: some 1e-7 m)
DELTA = 2e-6


def age(key):
    return int(key) >> 28


def decode_cache(keys, lam, count, decode):
    """{identity: (age, impulse[3])} of one env's cache: keys [cap] uint32, lam [3, cap]; decode: key -> identity"""
    return {decode(keys[c]): (age(keys[c]), lam[:, c]) for c in range(int(count))}


def contact_caches(g_warm, o_warm, ns, e):
    """env e of two oracle.physics_oracle.WarmState-like caches (.key [n, cap], .lam [n, 3, cap], .count [n]), the first in the
    kernel's key encoding, the second in the oracle's (ns = the scene's n_static): two dicts {identity: (age, impulse[3])}"""
    G = decode_cache(g_warm.key[e], g_warm.lam[e], g_warm.count[e], decode_kernel)
    O = decode_cache(o_warm.key[e], o_warm.lam[e], o_warm.count[e], lambda k: decode_oracle(k, ns))
    return G, O


def contact_sets(g_warm, o_warm, ns, e):
    """as contact_caches, without the ages: two dicts {identity: impulse[3]}"""
    G, O = contact_caches(g_warm, o_warm, ns, e)
    return {k: v[1] for k, v in G.items()}, {k: v[1] for k, v in O.items()}


def box_pair(identity):
    """the (body a, body b, box pair) part of an identity: the unit whose four contact slots its samples compete for"""
    return identity[:3]


def desc_with(desc, **fields):
    """a copy of a scene descriptor (a plain ctypes structure) with some fields replaced"""
    d = type(desc).from_buffer_copy(desc)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def oracle_list(desc, root_env, dof_env):
    """the oracle's contact list of one env's state: [(identity, separation)] in list order, and the count before the capacity cut"""
    ns = int(desc.n_static)
    con, total = po.contacts(desc, root_env, dof_env)
    keys = po.contact_keys(desc, root_env, dof_env)
    assert len(keys) == len(con)
    return [(decode_oracle(k, ns), float(s)) for k, s in zip(keys, con[:, 8])], total


def boundary_samples(desc, root_env, dof_env, thr, delta=DELTA, delta_rbox=None):
    """[(identity, separation)] of the samples with |sep - thr| < delta in the oracle's list at inclusion threshold thr + delta
    (delta_rbox, if given, instead of delta for the pairs of a robot box, whose pose comes out of the forward kinematics).  thr: the
    descriptor's contact offset, or 0 for an env whose list the capacity rule rebuilds (a list at contact_offset = delta does not
    overflow)."""
    dmax = max(delta, delta_rbox or 0.0)
    lst, total = oracle_list(desc_with(desc, contact_offset=thr + dmax), root_env, dof_env)
    assert total <= po.lib().sdxo_max_contacts(), total        # (the classifying list itself must be complete)
    return [(i, sep) for i, sep in lst
            if abs(sep - thr) < (delta_rbox if (delta_rbox is not None and i[0][0] == "rbox") else delta)]


def boundary_pairs(desc, root_env, dof_env, thr, delta=DELTA, delta_rbox=None):
    """the set of (body a, body b, box pair) that hold a boundary sample.  Per box pair, not per sample: the four slots of a pair are
    contested, so one sample that crosses the threshold can change which of its neighbours are listed."""
    return {box_pair(i) for i, _ in boundary_samples(desc, root_env, dof_env, thr, delta, delta_rbox)}
