"""Which stage-A kernel the ADER-DG units pick is pinned: tests/host/stage_a_selection.cpp prints, for every launch table (the five built
(dim, pde) pairs, the SymPy Euler set and a generated term set with position- / time-dependent terms and an ncp), every N in 2..8, n_picard in
{0, 1, 3} and variant in {0, 1, 2}, the kernel's name, whether the one-kernel step exists, the slab bytes and the size of the operator image, and
a hash of the lane tables of the reg / m8 kernels.  tests/golden/stage_a_selection.txt is that output from the library BEFORE the selection was
brought into one function (dg_inst.hip stage_a_kind): the name the profiles and bench.py trust, and the table builders, cannot drift unnoticed.

Lines differ from that library only where its launch refused the combination (it still printed a name for them; now the name is empty):
the golden holds an empty name there.  No device is needed: these are host functions of the launch tables."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "stage_a_selection.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_a_selection.txt")


def test_stage_a_selection_matches_the_pinned_table(tmp_path):
    import bench
    from exahype_amd import build
    from tests.test_user_pde import coupled_xt_ncp_system
    lib = os.path.dirname(build.build())
    sets = [("sympy_euler", bench.sympy_euler().build()), ("coupled_xt_ncp", coupled_xt_ncp_system().build())]
    exe = str(tmp_path / "stage_a_selection")
    r = subprocess.run([build._hipcc(), "-x", "hip", "--offload-arch=" + build.ARCH, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", build.CSRC, SRC, "-o", exe,
                        "-L", lib, "-lexahype_hip", "-ldl", "-Wl,-rpath," + lib], capture_output=True, text=True, env=build.compiler_env())
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + ["%s=%s" % s for s in sets], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got, want = r.stdout.splitlines(), open(GOLDEN).read().splitlines()
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not bad, "%d lines, golden %d; first differences:\n%s" % (len(got), len(want), "\n".join("got  %s\nwant %s" % b for b in bad[:5]))
