"""The launch plan of the "fleet_glb16" rollout form (csrc/rollout_glb16.hip: fleet_glb16_plan; CPU only).

Up to 64 controllers, every one with its OWN layer list and cap on the resident blocks, share a rollout launch: grid (workgroups
of the largest instance, instances); ONE kernel instance -- 16 tiles per layer if any list is wider than 128, else 8 --, ONE
dynamic-LDS size -- the largest of the instances' own -- and ONE workgroup size -- the rule of "glb16" (tests/test_glb16_pack.py:
workgroup_threads) with that LDS on all workgroups of the fleet.  Every instance keeps the R of a launch of its own.  The plan is
an ordinary function of libmppi_hip.so; a small C++ program linked against the library calls it."""
import os
import subprocess

import pytest

from tests.test_glb16_pack import lds_bytes, resident_blocks, stream_blocks, workgroup_threads
from tests.test_lds16_pack import LDS_LIMIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")

HARNESS = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace mppi {
struct NetDesc { int n_layers; int layers[8]; int max_width; int num_params; };
struct Lds16Net { int n_w; int img_f4; int mt[7]; int ks[7]; int off[7]; int boff[7]; int nout[7]; };
struct FleetGlbNet { Lds16Net net; int R; };
struct FleetGlb16Plan { int tiles, threads, grid_x, grid_y; size_t lds_bytes; };
FleetGlb16Plan fleet_glb16_plan(const NetDesc *nets, const int *caps, const int *Ks, int n, int cus);
FleetGlbNet fleet_glb16_net_of(const NetDesc &net, int cap);
Lds16Net glb16_net_of(const NetDesc &net);
}
// argv: cus, then per member "K,cap,layer,layer,..."
int main(int argc, char **argv)
{
  const int cus = atoi(argv[1]);
  std::vector<mppi::NetDesc> nets;
  std::vector<int> caps, Ks;
  for (int i = 2; i < argc; i++) {
    mppi::NetDesc net{};
    char *p = argv[i];
    Ks.push_back((int)strtol(p, &p, 10));
    caps.push_back((int)strtol(p + 1, &p, 10));
    while (*p == ',') net.layers[net.n_layers++] = (int)strtol(p + 1, &p, 10);
    nets.push_back(net);
  }
  const mppi::FleetGlb16Plan p = mppi::fleet_glb16_plan(nets.data(), caps.data(), Ks.data(), (int)Ks.size(), cus);
  printf("%d %d %d %d %zu\n", p.tiles, p.threads, p.grid_x, p.grid_y, p.lds_bytes);
  // every member's descriptor: R, and whether its offsets are those of the list alone
  for (size_t i = 0; i < nets.size(); i++) {
    const mppi::FleetGlbNet d = mppi::fleet_glb16_net_of(nets[i], caps[i]);
    const mppi::Lds16Net own = mppi::glb16_net_of(nets[i]);
    bool same = d.net.n_w == own.n_w && d.net.img_f4 == own.img_f4;
    for (int j = 0; j < 7; j++)
      same = same && d.net.mt[j] == own.mt[j] && d.net.ks[j] == own.ks[j] && d.net.off[j] == own.off[j] && d.net.boff[j] == own.boff[j] && d.net.nout[j] == own.nout[j];
    printf("%d %d\n", d.R, (int)same);
  }
  return 0;
}
"""

DEEP8 = [6, 20, 70, 9, 130, 33, 65, 4]
W128X4 = [6, 128, 128, 128, 128, 4]
# the nine lists of tests/test_glb16_gpu.py: NETS
NETS = [[6, 129, 4], [6, 256, 7, 4], [6, 200, 256, 4], [6, 256, 256, 4], [6, 197, 67, 4], [6, 16, 256, 4], DEEP8, W128X4, [6, 33, 97, 66, 4]]
CUS = [64, 256]
EMPTY = (0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from autorally_amd import build as B
    B.build()
    d = tmp_path_factory.mktemp("fleet_glb16_plan")
    src, exe = str(d / "plan.cpp"), str(d / "plan")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(members, cus):
        """members: (layers, K, cap) each -> (tiles, threads, grid x, grid y, LDS bytes), [(R, offsets are the list's own)]"""
        args = ["%d,%d,%s" % (K, cap, ",".join(map(str, layers))) for layers, K, cap in members]
        r = subprocess.run([exe, str(cus)] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.strip().split("\n")]
        return lines[0], lines[1:]
    return run


def fleet_threads(members, cus):
    """workgroup_threads of tests/test_glb16_pack.py with the launch's one LDS size (the largest of the members') and the launch's
    workgroups counted over the fleet: a workgroup serves one instance, so an instance of w waves brings ceil(w / waves per
    workgroup) of them.  Two waves per SIMD by the registers of either instance, 512 threads the largest workgroup of both."""
    by_lds = LDS_LIMIT // max(lds_bytes(layers, cap) for layers, _, cap in members)
    for threads in (256, 512):
        wpb = threads // 64
        if sum(-(-(K // 16) // wpb) for _, K, _ in members) <= min(by_lds, 4 * 2 // wpb) * cus:
            return threads
    return 512


def expected(members, cus):
    threads = fleet_threads(members, cus)
    tiles = 16 if any(max(layers[1:-1]) > 128 for layers, _, _ in members) else 8
    gx = -(-(max(K for _, K, _ in members) // 16) // (threads // 64))
    return (tiles, threads, gx, len(members), max(lds_bytes(layers, cap) for layers, _, cap in members))


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("layers", NETS, ids=lambda l: "-".join(map(str, l)))
def test_one_instance_is_the_plan_of_glb16(plan, layers, cus):
    for cap in (-1, 0, 3):
        for K in (64, 192, 1984, 4096, 16384, 65536 + 64):
            got, descs = plan([(layers, K, cap)], cus)
            threads = workgroup_threads(layers, K, cus, cap)
            tiles = 16 if max(layers[1:-1]) > 128 else 8
            assert got == (tiles, threads, -(-(K // 16) // (threads // 64)), 1, lds_bytes(layers, cap)), (layers, K, cus, cap, got)
            assert descs == [(resident_blocks(layers, cap), 1)]


NARROW = [[6, 5, 7, 4], [6, 32, 32, 4], [6, 33, 97, 66, 4], W128X4, [6, 64, 64, 64, 64, 4]]
WIDE = [[6, 33, 97, 66, 4], [6, 197, 67, 4], [6, 16, 256, 4], [6, 129, 4], [6, 256, 256, 4]]
KSETS = [(192, 64, 4096, 1984, 64), (64, 64, 64, 64, 4096), (1920,) * 5, (64,) * 5, (4096,) * 5]


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("lists", [NARROW, WIDE], ids=["narrow", "wide"])
def test_the_plan_of_a_mixed_fleet(plan, lists, cus):
    seen = set()
    fleets = [[(l, K, -1) for l, K in zip(lists, Ks)] for Ks in KSETS]
    fleets.append([(lists[i % 5], 1920, -1) for i in range(16)])
    fleets.append([(lists[i % 5], 4096, -1) for i in range(64)])
    fleets.append([(lists[i % 5], 64, -1) for i in range(64)])
    for members in fleets:
        got, descs = plan(members, cus)
        tiles, threads, gx, gy, nbytes = got
        assert got == expected(members, cus), (members, got)
        # the tile class is 16 exactly when a member is wider than 128
        assert tiles == (16 if lists is WIDE else 8)
        # the LDS is the largest of the members', and within the limit
        assert nbytes == max(lds_bytes(l, c) for l, _, c in members) <= LDS_LIMIT
        wpb = threads // 64
        kmax = max(K for _, K, _ in members)
        assert gx * wpb * 16 >= kmax > (gx - 1) * wpb * 16, "grid x covers the largest K wherever it stands"
        assert gy == len(members)
        # every member keeps the R and the offsets of a launch of its own
        assert descs == [(resident_blocks(l, c), 1) for l, _, c in members]
        # the order of the members does not matter
        back, back_descs = plan(members[::-1], cus)
        assert back == got and back_descs == descs[::-1]
        seen.add(threads)
    print("FLEET_GLB16 plan %s on %d CUs: workgroup sizes %s" % ("wide" if lists is WIDE else "narrow", cus, sorted(seen)))
    if cus == 64:
        assert seen == {256, 512}, "the fleets of this test reach both workgroup sizes"


@pytest.mark.parametrize("cus", CUS)
def test_a_wide_member_anywhere_makes_it_the_16_tile_launch(plan, cus):
    narrow = [([6, 32, 32, 4], 64, -1), ([6, 128, 128, 4], 192, -1), ([6, 5, 7, 4], 64, -1)]
    assert plan(narrow, cus)[0][0] == 8
    for at in range(4):
        for wide in ([6, 129, 4], [6, 16, 256, 4]):
            members = narrow[:at] + [(wide, 64, -1)] + narrow[at:]
            got, _ = plan(members, cus)
            assert got == expected(members, cus) and got[0] == 16, (members, got)


@pytest.mark.parametrize("cus", CUS)
def test_a_members_cap_changes_only_its_own_R_and_the_maximum(plan, cus):
    lists = [[6, 32, 32, 4], [6, 33, 97, 66, 4], W128X4, [6, 64, 64, 64, 64, 4], [6, 5, 7, 4]]
    Ks = (64, 1984, 64, 192, 64)
    free = [(l, K, -1) for l, K in zip(lists, Ks)]
    got0, descs0 = plan(free, cus)
    assert got0 == expected(free, cus)
    # W128X4 streams by default and holds the maximum: a cap on another member changes that member's R alone
    assert got0[4] == lds_bytes(W128X4) and resident_blocks(W128X4) < stream_blocks(W128X4)
    for caps in ((0, 1, -1, 3, 17), (3, -1, -1, 0, 0), (-1, -1, 5, -1, -1), (0, 0, 0, 0, 0), (-1, 2, 100, -1, 1)):
        members = [(l, K, c) for (l, K, _), c in zip(free, caps)]
        got, descs = plan(members, cus)
        assert got == expected(members, cus), (caps, got)
        assert descs == [(resident_blocks(l, c), 1) for l, _, c in members]
        for i, c in enumerate(caps):
            if c < 0:
                assert descs[i] == descs0[i]
        assert got[4] == max(lds_bytes(l, c) for l, _, c in members)
        if caps[2] < 0:
            assert got[4] == got0[4]
        else:
            assert got[4] < got0[4]


def test_an_empty_plan_where_there_is_no_launch(plan):
    ok = ([6, 32, 32, 4], 64, -1)
    assert plan([], 256)[0] == EMPTY
    assert plan([ok] * 65, 256)[0] == EMPTY
    assert plan([ok, ([6, 32, 32, 4], 0, -1)], 256)[0] == EMPTY
    assert plan([ok, ([6, 4], 64, -1)], 256)[0] == EMPTY
    assert plan([([6, 257, 4], 64, -1), ok], 256)[0] == EMPTY
    assert plan([ok] * 64, 256)[0] != EMPTY
    assert plan([ok, ([6, 256, 4], 64, -1)], 256)[0] != EMPTY
