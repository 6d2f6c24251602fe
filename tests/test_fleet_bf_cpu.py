"""The launch plan of the "fleet_bf" rollout form (csrc/rollout_fleet_bf.hip: fleet_bf_plan; CPU only).

Up to 64 controllers of the basis-function model share a rollout launch: one, two or three waves per workgroup of 64 rollouts,
grid x = the 64-rollout groups of the largest instance, grid y = the instances.  The wave count follows the rule of one handle
(csrc/abi_forms.hip: form_of) with the groups counted over the fleet, G = sum K / 64: three waves while 3 G <= simds, else two
while G <= simds, else one; a forced count (the "fleet_bf_w<N>" names) overrides it.  The plan is an ordinary function of
libmppi_hip.so; a small C++ program linked against the library calls it.  (What needs a handle -- the names, the refusals -- is
tests/test_fleet_bf_gpu.py's: without a device no handle exists.)"""
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
struct FleetBfPlan { int waves, threads, grid_x, grid_y; };
FleetBfPlan fleet_bf_plan(const int *Ks, int n, int simds, int forced_waves);
}
// argv: simds, forced_waves, the Ks
int main(int argc, char **argv)
{
  std::vector<int> Ks;
  for (int i = 3; i < argc; i++) Ks.push_back(atoi(argv[i]));
  const mppi::FleetBfPlan p = mppi::fleet_bf_plan(Ks.data(), (int)Ks.size(), atoi(argv[1]), atoi(argv[2]));
  printf("%d %d %d %d\n", p.waves, p.threads, p.grid_x, p.grid_y);
  return 0;
}
"""

SIMDS = 1024  # MI355X: 256 CUs of 4
FLEETS = [(192, 64, 128, 192, 64), (4096, 64), (64, 4096), (2560,) * 4, (2560,) * 16, (2560,) * 64, (64,) * 64, (64,)]
EMPTY = (0, 0, 0, 0)


def rule(Ks, simds):
    """form_of's rule for one handle, the groups counted over the fleet"""
    G = sum(K // 64 for K in Ks)
    return 3 if 3 * G <= simds else (2 if G <= simds else 1)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from autorally_amd import build as B
    B.build()
    d = tmp_path_factory.mktemp("fleet_bf_plan")
    src, exe = str(d / "plan.cpp"), str(d / "plan")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(Ks, simds=SIMDS, forced=0):
        r = subprocess.run([exe, str(simds), str(forced)] + [str(k) for k in Ks], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return tuple(int(x) for x in r.stdout.split())
    return run


def test_the_plan_of_a_fleet(plan):
    for Ks in FLEETS:
        got = plan(Ks)
        w = rule(Ks, SIMDS)
        assert got == (w, 64 * w, max(Ks) // 64, len(Ks)), (Ks, got)
        assert plan(Ks[::-1]) == got, "the order of the instances does not matter"


def test_the_wave_counts_of_the_fleets_of_the_reference_size(plan):
    """K = 2560 (path_integral_bf): 4 handles are 160 groups, 16 are 640, 64 are 2560 -- on 1024 SIMDs three, two and one wave."""
    for n, groups, waves in ((4, 160, 3), (16, 640, 2), (64, 2560, 1)):
        Ks = (2560,) * n
        assert sum(K // 64 for K in Ks) == groups
        assert plan(Ks) == (waves, 64 * waves, 40, n), n


def test_one_handle_gets_the_choice_of_a_single_solve(plan):
    """n = 1: form_of's thresholds for that handle -- 3 (K / 64) <= simds: three waves; K / 64 <= simds: two; else one."""
    for simds in (1024, 12):
        for K in (64, 64 * (simds // 3), 64 * (simds // 3 + 1), 64 * simds, 64 * (simds + 1)):
            G = K // 64
            w = 3 if 3 * G <= simds else (2 if 2 * G <= 2 * simds else 1)
            assert plan((K,), simds) == (w, 64 * w, G, 1), (K, simds)


def test_the_boundaries_on_both_sides(plan):
    """simds = 12: G = 4 is the last fleet with three waves, G = 12 the last with two."""
    simds = 12
    for Ks, waves in (((128, 64, 64), 3),        # G = 4 = simds / 3
                      ((128, 128, 64), 2),       # G = 5
                      ((256, 256, 192, 64), 2),  # G = 12 = simds
                      ((256, 256, 192, 128), 1),  # G = 13
                      ((64,) * 4, 3), ((64,) * 5, 2), ((64,) * 12, 2), ((64,) * 13, 1)):
        got = plan(Ks, simds)
        assert got == (waves, 64 * waves, max(Ks) // 64, len(Ks)), (Ks, got)
        assert plan(Ks[::-1], simds) == got


def test_a_forced_wave_count(plan):
    for Ks in FLEETS:
        for forced in (1, 2, 3):
            assert plan(Ks, SIMDS, forced) == (forced, 64 * forced, max(Ks) // 64, len(Ks)), (Ks, forced)
            assert plan(Ks[::-1], SIMDS, forced) == plan(Ks, SIMDS, forced)


def test_an_empty_plan_where_there_is_no_launch(plan):
    assert plan([]) == EMPTY
    assert plan([64] * 65) == EMPTY
    assert plan([64, 0]) == EMPTY
    assert plan([64, 208]) == EMPTY, "a K that is no multiple of 64"
    assert plan([64, 64], SIMDS, 4) == EMPTY, "no such wave count"
    assert plan([64, 64], SIMDS, -1) == EMPTY
    assert plan([64] * 64) != EMPTY
    for forced in (0, 1, 2, 3):
        assert plan([64, 208], SIMDS, forced) == EMPTY and plan([64] * 65, SIMDS, forced) == EMPTY
