"""CPU (-m "not gpu"): the emulator libraries are rebuilt when a file they are compiled from is newer.  Every file that the sources of
tests/hipemu's build() / build_sim() reach through their #include "..." lines, inside seqdex_amd/csrc and include/, must be in the list
the build compares the library against - a header missing from it (sdx_kernels.h, say, or one of sdx_physics.hip's sdx_phys_*.h) means
tests that run a stale library.  Reads text only: no compiler."""
import os
import re

from tests import hipemu

INCLUDE_DIR = os.path.join(hipemu.ROOT, "include")


def reached(sources):
    """files under csrc / include that `sources` include, directly or through each other (all #include "..." lines, whatever #if they sit in)"""
    seen, todo = set(), [s for s in sources if s.startswith(hipemu.CSRC)]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), flags=re.M):
            for base in (os.path.dirname(f), hipemu.CSRC, INCLUDE_DIR):
                path = os.path.normpath(os.path.join(base, name))
                if os.path.isfile(path) and (path.startswith(hipemu.CSRC) or path.startswith(INCLUDE_DIR)):
                    todo.append(path)
                    break
    return seen


def test_emulator_builds_list_every_included_file():
    physics = reached([os.path.join(hipemu.CSRC, "sdx_physics.hip")])
    names = {os.path.basename(f) for f in physics}
    assert {"sdx_kernels.h", "sdx_common.h", "seqdex.h", "sdx_phys_lds.h", "sdx_phys_solve.h"} <= names   # the walk itself works
    for what, sources, deps in (("build", hipemu._SRCS, hipemu.build_deps()), ("build_sim", hipemu._SIM_SRCS, hipemu.build_sim_deps())):
        files = reached(sources)
        assert physics <= files, what   # both libraries compile the physics unit
        missing = sorted(os.path.relpath(f, hipemu.ROOT) for f in files - set(deps))
        assert not missing, "%s(): not in its dependency list: %s" % (what, missing)
