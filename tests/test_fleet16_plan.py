"""The launch plan of the "fleet16" rollout form (csrc/rollout_fleet16.hip: fleet16_plan; CPU only).

Up to 64 controllers of one layer list share a rollout launch: grid (workgroups of the largest instance, instances), ONE
workgroup size for the launch -- the rule of "lds16" (tests/test_lds16_pack.py: workgroup_threads) on all workgroups of the
fleet -- and the image of "lds16" as the workgroup's dynamic LDS.  The plan is an ordinary function of libmppi_hip.so; a small
C++ program linked against the library calls it."""
import os
import subprocess

import pytest

from tests.test_lds16_pack import LDS_LIMIT, image_quads, workgroup_threads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")

HARNESS = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace mppi {
struct NetDesc { int n_layers; int layers[8]; int max_width; int num_params; };
struct Fleet16Plan { int threads, grid_x, grid_y; size_t lds_bytes; };
Fleet16Plan fleet16_plan(const NetDesc &net, const int *Ks, int n, int cus);
size_t lds16_lds_bytes(const NetDesc &net);
int lds16_block_threads(const NetDesc &net, int K, int cus);
}
// argv: cus, the layer list, "/", the Ks
int main(int argc, char **argv)
{
  mppi::NetDesc net{};
  const int cus = atoi(argv[1]);
  int i = 2;
  for (; i < argc && argv[i][0] != '/'; i++) net.layers[net.n_layers++] = atoi(argv[i]);
  std::vector<int> Ks;
  for (i++; i < argc; i++) Ks.push_back(atoi(argv[i]));
  const mppi::Fleet16Plan p = mppi::fleet16_plan(net, Ks.data(), (int)Ks.size(), cus);
  printf("%d %d %d %zu %zu %d\n", p.threads, p.grid_x, p.grid_y, p.lds_bytes, mppi::lds16_lds_bytes(net),
         Ks.empty() ? 0 : mppi::lds16_block_threads(net, Ks[0], cus));
  return 0;
}
"""

LISTS = [[6, 5, 7, 4], [6, 32, 32, 4], [6, 64, 64, 64, 64, 4], [6, 33, 97, 66, 4], [6, 128, 128, 128, 4]]
CUS = [64, 256]
FLEETS = [(192, 64, 4096, 1984, 64), (4096, 64), (64, 4096), (1920,) * 16, (4096,) * 64, (64,) * 64, (1984, 4096, 1984)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from autorally_amd import build as B
    B.build()
    d = tmp_path_factory.mktemp("fleet16_plan")
    src, exe = str(d / "plan.cpp"), str(d / "plan")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(layers, Ks, cus):
        """-> (threads, grid x, grid y, LDS bytes), lds16_lds_bytes, lds16_block_threads(net, Ks[0], cus)"""
        r = subprocess.run([exe, str(cus)] + [str(x) for x in layers] + ["/"] + [str(k) for k in Ks], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        v = [int(x) for x in r.stdout.split()]
        return tuple(v[:4]), v[4], v[5]
    return run


def fleet_threads(layers, Ks, cus):
    """workgroup_threads of tests/test_lds16_pack.py with the launch's workgroups counted over the fleet: a workgroup serves one
    instance, so an instance of w waves brings ceil(w / waves per workgroup) of them."""
    wide = max(layers[1:-1]) > 64
    wps, largest = (3, 512) if wide else (4, 1024)
    by_lds = LDS_LIMIT // (image_quads(layers) * 16)
    for threads in (256, 512, 1024):
        if threads > largest:
            break
        wpb = threads // 64
        if sum(-(-(K // 16) // wpb) for K in Ks) <= min(by_lds, 4 * wps // wpb) * cus:
            return threads
    return largest


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("layers", LISTS, ids=lambda l: "-".join(map(str, l)))
def test_one_instance_is_the_plan_of_lds16(plan, layers, cus):
    for K in (64, 192, 1984, 4096, 16384, 65536 + 64):
        got, lds, single = plan(layers, [K], cus)
        threads = workgroup_threads(layers, K, cus)
        assert single == threads
        assert got == (threads, -(-(K // 16) // (threads // 64)), 1, image_quads(layers) * 16), (layers, K, cus, got)
        assert got[3] == lds


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("layers", LISTS, ids=lambda l: "-".join(map(str, l)))
def test_the_plan_of_a_fleet(plan, layers, cus):
    wide = max(layers[1:-1]) > 64
    seen = set()
    for Ks in FLEETS:
        got, lds, _ = plan(layers, Ks, cus)
        threads, gx, gy, nbytes = got
        assert threads in ((256, 512) if wide else (256, 512, 1024)), got
        assert threads == fleet_threads(layers, Ks, cus), (Ks, got)
        wpb = threads // 64
        assert gx == -(-(max(Ks) // 16) // wpb), "grid x covers the largest K wherever it stands"
        assert gx * wpb * 16 >= max(Ks) > (gx - 1) * wpb * 16
        assert gy == len(Ks)
        assert nbytes == lds == image_quads(layers) * 16 <= LDS_LIMIT
        # the order of the instances does not matter
        assert plan(layers, Ks[::-1], cus)[0] == got
        seen.add(threads)
    print("FLEET16 plan %s on %d CUs: workgroup sizes %s" % ("-".join(map(str, layers)), cus, sorted(seen)))
    if cus == 64:
        assert len(seen) >= 2, "the fleets of this test reach more than one workgroup size"


def test_an_empty_plan_where_there_is_no_launch(plan):
    empty = (0, 0, 0, 0)
    for layers in ([6, 129, 4], [6, 4], [6, 128, 128, 128, 128, 4]):  # what lds16 refuses: too wide, no hidden layer, too big an image
        assert plan(layers, [64, 64], 256)[0] == empty, layers
    assert plan([6, 32, 32, 4], [], 256)[0] == empty
    assert plan([6, 32, 32, 4], [64] * 65, 256)[0] == empty
    assert plan([6, 32, 32, 4], [64, 0], 256)[0] == empty
    assert plan([6, 32, 32, 4], [64] * 64, 256)[0] != empty


def test_the_host_layer_has_the_fleet_calls(tmp_path):
    """startControlFleet / finishControlFleet of host/mppi_controller_hip.hpp beside startControlPair: instantiated for the network
    controller and linked against the library."""
    src, exe = str(tmp_path / "fleet_host.cpp"), str(tmp_path / "fleet_host")
    with open(src, "w") as f:
        f.write('#include "mppi_controller_hip.hpp"\n'
                "using C = mppi_host::MPPIController;\n"
                "void (*start)(C *const *, int, const float *) = &C::startControlFleet;\n"
                "void (*finish)(C *const *, int) = &C::finishControlFleet;\n"
                "int main() { C::startControlFleet(nullptr, 0, nullptr); C::finishControlFleet(nullptr, 0); return start == nullptr || finish == nullptr; }\n")
    from autorally_amd import build as B
    B.build()
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DMPPI_NPZ_ZLIB", "-I" + os.path.join(PKG, "host"), src, "-o", exe,
                           "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG, "-lz", "-lpthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0   # an empty fleet: nothing is called, no device is needed
