"""Census of the branch-rich PPO test data (tests/helpers/ppo_branch_data.py) with the oracle alone, on the CPU: for every shape and case of
tests/test_gpu_ppo_branches.py the counts of every class of decision, the smallest distance of any decision from its boundary, and whether
the conditions of the tests hold; and how far the fp32 oracle lands from the same oracle run in float64 (parameters after the update), the
yardstick for the parameter bounds of the tests: max(bound of test_update_matches_autograd_adam, 4 x that difference).

    python tools/ppo_branch_census.py [--out profiles/ppo_branch_tests_bounds.txt]"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from helpers import ppo_branch_data as BD  # noqa: E402
from oracle.ppo_oracle import census_summary  # noqa: E402

CASES = {"defaults": {}, "clip_value_0": dict(clip_value=0), "truncate_grads_0": dict(truncate_grads=0),
         "normalize_advantage_0": dict(normalize_advantage=0), "cv_normalize_input_0": dict(cv_normalize_input=0),
         "entropy_coef_0.02": dict(entropy_coef=0.02), "bounds_loss_coef_0.05": dict(bounds_loss_coef=0.05)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["census of the branch-rich data, oracle alone (tools/ppo_branch_census.py); required: >= %d rows per class, >= %d steps per class,"
             % (BD.MIN_ROWS, BD.MIN_STEPS), "margins >= %r" % (BD.MARGINS,), ""]
    todo = [(16, 4, c) for c in CASES] + [(48, 48, c) for c in CASES] + [(16, 2, "defaults"), (16, 8, "defaults")]
    ok = True
    for n, mb, case in todo:
        orc0, ds = BD.branch_dataset(n, mb, **CASES[case])
        orc, o64 = copy.deepcopy(orc0), copy.deepcopy(orc0)
        s = census_summary(orc.update({k: v.clone() for k, v in ds.items()})["census"])
        for m in (o64.actor, o64.critic, o64.cv):
            m.double()
        o64.logstd.data = o64.logstd.data.double()
        o64.update({k: v.double() for k, v in ds.items()})
        d_ac = float((orc.ac_flat().double() - o64.ac_flat()).abs().max())
        d_cv = float((orc.cv_flat().double() - o64.cv_flat()).abs().max())
        bad = BD.census_violations(s, clip_value=bool(CASES[case].get("clip_value", 1)), minibatch=mb)
        ok = ok and not bad
        lines += ["%d envs, minibatch %d, %s: %s" % (n, mb, case, "conditions hold" if not bad else "VIOLATED: %s" % bad),
                  "  rows    " + ", ".join("%s %d" % kv for kv in s["rows"].items()),
                  "  steps   " + ", ".join("%s %d" % kv for kv in s["steps"].items()),
                  "  margins " + ", ".join("%s %.3g" % kv for kv in s["margins"].items()),
                  "  fp32 oracle against float64 oracle, parameters after the update: max |d ac| %.2e, max |d cv| %.2e" % (d_ac, d_cv)]
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        open(a.out, "w").write(txt)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
