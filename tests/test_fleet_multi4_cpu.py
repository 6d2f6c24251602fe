"""The launch plan of the "fleet_multi4" rollout form (csrc/rollout_fleet_multi.hip: fleet_multi_plan; CPU only).

Up to 64 controllers of one standard network share a rollout launch: eight waves per workgroup of 64 rollouts, grid x = the
64-rollout groups of the largest instance, grid y = the instances.  The plan is an ordinary function of libmppi_hip.so; a small
C++ program linked against the library calls it.  (What needs a handle -- the name, the refusals -- is tests/test_fleet_multi4_gpu.py's:
without a device no handle exists.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace mppi {
struct FleetMultiPlan { int threads, grid_x, grid_y; };
FleetMultiPlan fleet_multi_plan(int hidden, int n_hidden, const int *Ks, int n);
}
// argv: hidden, n_hidden, the Ks
int main(int argc, char **argv)
{
  std::vector<int> Ks;
  for (int i = 3; i < argc; i++) Ks.push_back(atoi(argv[i]));
  const mppi::FleetMultiPlan p = mppi::fleet_multi_plan(atoi(argv[1]), atoi(argv[2]), Ks.data(), (int)Ks.size());
  printf("%d %d %d\n", p.threads, p.grid_x, p.grid_y);
  return 0;
}
"""

SHAPES = [(32, 2), (32, 4), (64, 2)]
FLEETS = [(192, 64, 128, 192, 64), (4096, 64), (64, 4096), (1920,) * 16, (4096,) * 64, (64,) * 64, (64,)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from autorally_amd import build as B
    B.build()
    d = tmp_path_factory.mktemp("fleet_multi_plan")
    src, exe = str(d / "plan.cpp"), str(d / "plan")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(hidden, n_hidden, Ks):
        r = subprocess.run([exe, str(hidden), str(n_hidden)] + [str(k) for k in Ks], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return tuple(int(x) for x in r.stdout.split())
    return run


@pytest.mark.parametrize("hidden,n_hidden", SHAPES)
def test_the_plan_of_a_fleet(plan, hidden, n_hidden):
    for Ks in FLEETS:
        got = plan(hidden, n_hidden, Ks)
        assert got == (8 * 64, max(Ks) // 64, len(Ks)), (Ks, got)
        assert plan(hidden, n_hidden, Ks[::-1]) == got, "the order of the instances does not matter"


def test_an_empty_plan_where_there_is_no_launch(plan):
    empty = (0, 0, 0)
    for hidden, n_hidden in ((64, 4), (48, 2), (32, 3), (128, 2)):   # shapes the multi form does not have
        assert plan(hidden, n_hidden, [64, 64]) == empty, (hidden, n_hidden)
    assert plan(32, 2, []) == empty
    assert plan(32, 2, [64] * 65) == empty
    assert plan(32, 2, [64, 0]) == empty
    assert plan(32, 2, [64, 208]) == empty, "a K that is no multiple of 64"
    assert plan(32, 2, [64] * 64) != empty
