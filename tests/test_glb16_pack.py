"""The weight image, the residency rule and the workgroup rule of the "glb16" rollout form (csrc/rollout_glb16.hip,
csrc/abi_pack.hip: pack_glb16_weights; CPU only).

The packer and the rules are ordinary functions of libmppi_hip.so; a small C++ program linked against the library calls them (no
export of the C ABI is involved).  The image is "lds16"'s (tests/test_lds16_pack.py has the layout) with up to 16 tiles per layer:
bias quads, layer 0 half blocks -- the HEAD, always in LDS --, then one stream of 1 KB blocks over all later layers in the order of
their use, then AHEAD blocks of zeros.  Of the stream R blocks are resident:
  R = min(stream blocks with the zero blocks, floor((160 KB - head bytes) / 1 KB), the cap of "glb16_r<N>")."""
import os
import subprocess

import numpy as np
import pytest

from autorally_amd import params as P
from tests.test_lds16_pack import LDS_LIMIT, TANH_SCALE, _block_index, _neuron, _tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")
AHEAD = 2       # csrc/mppi_kernels.hpp: kGlb16Ahead (blocks)
LDS16_AHEAD = 2  # csrc/rollout_lds16.hip: kLds16Ahead

HARNESS = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace mppi {
struct NetDesc { int n_layers; int layers[8]; int max_width; int num_params; };
struct Lds16Net { int n_w; int img_f4; int mt[7]; int ks[7]; int off[7]; int boff[7]; int nout[7]; };
Lds16Net glb16_net_of(const NetDesc &net);
bool glb16_supported(const NetDesc &net);
int glb16_pack_floats(const NetDesc &net);
size_t glb16_head_bytes(const NetDesc &net);
int glb16_stream_blocks(const NetDesc &net);
int glb16_resident_blocks(const NetDesc &net, int cap);
size_t glb16_lds_bytes(const NetDesc &net, int cap);
size_t glb16_lds_limit();
int glb16_block_threads(const NetDesc &net, int K, int cus, int cap);
int lds16_pack_floats(const NetDesc &net);
}
namespace mppi_abi {
std::vector<float> pack_glb16_weights(const std::vector<float> &theta, const mppi::NetDesc &net);
std::vector<float> pack_lds16_weights(const std::vector<float> &theta, const mppi::NetDesc &net);
}
static int dump(const char *path, const std::vector<float> &v)
{
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(v.data(), 4, v.size(), f) != v.size()) return 3;
  fclose(f);
  return 0;
}
int main(int argc, char **argv)
{
  // argv: theta file | "-cap,K,cus", image file, lds16 image file, layers...
  mppi::NetDesc net{};
  net.n_layers = argc - 4;
  for (int i = 0; i < net.n_layers; i++) net.layers[i] = atoi(argv[4 + i]);
  for (int i = 0; i + 1 < net.n_layers; i++) net.num_params += (net.layers[i] + 1) * net.layers[i + 1];
  printf("%d %d %zu %d %zu\n", (int)mppi::glb16_supported(net), mppi::glb16_pack_floats(net), mppi::glb16_head_bytes(net),
         mppi::glb16_stream_blocks(net), mppi::glb16_lds_limit());
  if (argv[1][0] == '-') {  // the rules: R, LDS bytes and the workgroup under a cap
    int cap = 0, K = 0, cus = 0;
    if (sscanf(argv[1] + 1, "%d,%d,%d", &cap, &K, &cus) != 3) return 4;
    printf("%d %zu %d\n", mppi::glb16_resident_blocks(net, cap), mppi::glb16_lds_bytes(net, cap), mppi::glb16_block_threads(net, K, cus, cap));
    return 0;
  }
  const mppi::Lds16Net d = mppi::glb16_net_of(net);
  printf("%d %d", d.n_w, d.img_f4);
  for (int j = 0; j < d.n_w; j++) printf(" %d %d %d %d %d", d.mt[j], d.ks[j], d.off[j], d.boff[j], d.nout[j]);
  printf("\n%d\n", mppi::lds16_pack_floats(net));
  std::vector<float> theta(net.num_params);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(theta.data(), 4, theta.size(), f) != theta.size()) return 2;
  fclose(f);
  if (int rc = dump(argv[2], mppi_abi::pack_glb16_weights(theta, net))) return rc;
  return dump(argv[3], mppi_abi::pack_lds16_weights(theta, net));
}
"""


@pytest.fixture(scope="module")
def glb16_packer(tmp_path_factory):
    from autorally_amd import build as B
    B.build()
    d = tmp_path_factory.mktemp("glb16_pack")
    src, exe = str(d / "pack.cpp"), str(d / "pack")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(layers, theta=None, cap=-1, K=0, cus=0):
        """-> (supported, pack floats, head bytes, stream blocks, the limit), then
        without theta: (R, LDS bytes, threads per workgroup) under `cap`; with theta: Lds16Net, image, lds16's image"""
        tin, tout, tout16 = str(d / "theta.bin"), str(d / "image.bin"), str(d / "image16.bin")
        if theta is not None:
            np.asarray(theta, np.float32).tofile(tin)
        first = tin if theta is not None else "-%d,%d,%d" % (cap, K, cus)
        r = subprocess.run([exe, first, tout, tout16] + [str(x) for x in layers], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        lines = r.stdout.split("\n")
        cap_line = tuple(int(x) for x in lines[0].split())
        if theta is None:
            return cap_line, tuple(int(x) for x in lines[1].split())
        return cap_line, [int(x) for x in lines[1].split()], np.fromfile(tout, np.float32), np.fromfile(tout16, np.float32)
    return run


def head_quads(layers):
    mt = _tiles(layers)
    return 4 * sum(mt[:-1]) + 1 + 32 * mt[0]


def stream_blocks(layers):
    mt = _tiles(layers)
    return sum(a * b for a, b in zip(mt[1:], mt[:-1])) + AHEAD


def image_quads(layers):
    return head_quads(layers) + 64 * stream_blocks(layers)


def resident_blocks(layers, cap=-1):
    r = min(stream_blocks(layers), (LDS_LIMIT - 16 * head_quads(layers)) // 1024)
    return r if cap < 0 else min(r, cap)


def lds_bytes(layers, cap=-1):
    return 16 * head_quads(layers) + 1024 * resident_blocks(layers, cap)


def workgroup_threads(layers, K, cus, cap=-1):
    """lds16's rule on this form's LDS request and instances: the smaller of 256 / 512 threads for which every workgroup is
    resident at once -- floor(limit / requested bytes) workgroups per CU by the LDS, two waves per SIMD by the registers of
    either instance -- else 512."""
    waves = K // 16
    by_lds = LDS_LIMIT // lds_bytes(layers, cap)
    for threads in (256, 512):
        wpb = threads // 64
        if -(-waves // wpb) <= min(by_lds, 4 * 2 // wpb) * cus:
            return threads
    return 512


def expected_image(layers, theta):
    """every weight at its tile, row, k-step and lane, every bias at its slot, zeros elsewhere: [quad][component]"""
    mt, n_w = _tiles(layers), len(layers) - 1
    want = np.zeros((image_quads(layers), 4), np.float32)
    boff, woff, toff = 0, 4 * sum(mt[:-1]) + 1, 0
    offs = []
    for j, (nin, nout) in enumerate(zip(layers[:-1], layers[1:])):
        W = theta[toff:toff + nin * nout].reshape(nout, nin)
        b = theta[toff + nin * nout:toff + nin * nout + nout]
        last = j == n_w - 1
        offs.append([mt[j], 2 if j == 0 else 4 * mt[j - 1], woff, boff, nout])
        if last:
            want[boff] = b
        else:
            for n in range(nout):
                m, r, g = n // 16, (n % 16) // 4, n % 4
                want[boff + 4 * m + g, r] = b[n] * TANH_SCALE
        for m in range(mt[j]):
            for lane in range(64):
                row, kk = lane & 15, lane >> 4
                n = _neuron(m, row, last)
                if n >= nout:
                    continue
                if j == 0:
                    half = want[woff + 32 * m:woff + 32 * (m + 1)].reshape(64, 2)  # float2 per lane
                    for c in range(2):
                        if 4 * c + kk < nin:
                            half[lane, c] = W[n, 4 * c + kk]
                    continue
                for mi in range(mt[j - 1]):
                    blk = woff + 64 * _block_index(m, mi, mt[j], mt[j - 1])
                    k = 16 * mi + 4 * np.arange(4) + kk  # k-step 4 mi + c, k-slot kk
                    ok = k < nin
                    want[blk + lane, ok] = W[n, k[ok]]
        boff += 1 if last else 4 * mt[j]
        woff += 32 * mt[0] if j == 0 else 64 * mt[j] * mt[j - 1]
        toff += nin * nout + nout
    assert woff + 64 * AHEAD == image_quads(layers)
    return want, offs


W128x4 = [6, 128, 128, 128, 128, 4]
LISTS = [[6, 129, 4], [6, 256, 7, 4], [6, 200, 256, 4], [6, 256, 256, 4], [6, 16, 256, 4], [6, 20, 70, 9, 130, 33, 65, 4], W128x4,
         [6, 48, 48, 4]]


@pytest.mark.parametrize("layers", LISTS, ids=lambda l: "-".join(map(str, l)))
def test_every_weight_at_its_tile_row_kstep_and_lane_and_zeros_elsewhere(glb16_packer, layers):
    layers, theta = P.synthetic_model(layers, seed=9)
    theta = np.asarray(theta, np.float32)
    assert np.all(theta != 0.0)
    cap, desc, img, img16 = glb16_packer(layers, theta)
    n_w = len(layers) - 1
    assert cap == (1, image_quads(layers) * 4, head_quads(layers) * 16, stream_blocks(layers), LDS_LIMIT), cap
    assert img.size == image_quads(layers) * 4
    want, offs = expected_image(layers, theta)
    assert desc[:2] == [n_w, image_quads(layers)]
    assert [desc[2 + 5 * j:7 + 5 * j] for j in range(n_w)] == offs
    assert offs[1][2] == head_quads(layers), "the stream begins behind the head"
    img = img.reshape(-1, 4)
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    assert not np.any(img[-64 * AHEAD:])
    # every weight of the hidden layers once, the output layer's four times (rows 4 g' + o), 4 + hidden biases
    hidden = sum((nin + 1) * nout for nin, nout in zip(layers[:-2], layers[1:-1]))
    assert int(np.count_nonzero(img)) == hidden + 4 * 4 * layers[-2] + 4
    # where pack_lds16_weights has an image (hidden widths up to 128), it is this image float for float up to the zero blocks
    if max(layers[1:-1]) <= 128:
        body = image_quads(layers) * 4 - 256 * AHEAD
        assert img16.size == body + 256 * LDS16_AHEAD
        np.testing.assert_array_equal(img16[:body].view(np.uint32), img.reshape(-1)[:body].view(np.uint32))
        assert not np.any(img16[body:])
        if AHEAD == LDS16_AHEAD:
            np.testing.assert_array_equal(img16.view(np.uint32), img.reshape(-1).view(np.uint32))
    else:
        assert img16.size == 0


def test_the_residency_rule(glb16_packer):
    """Head bytes, R without a cap, under cap 0, cap 1 and a cap beyond capacity; the request never passes 160 KB."""
    for layers in LISTS + [[6, 256, 256, 256, 256, 256, 256, 4], [6, 1, 4], [6, 128, 128, 128, 4]]:
        cap_line, _ = glb16_packer(layers)
        assert cap_line[2] == 16 * head_quads(layers) <= 14 * 1024 + 256, (layers, cap_line)
        for cap in (-1, 0, 1, 10 ** 6):
            _, (R, nbytes, _) = glb16_packer(layers, cap=cap, K=1920, cus=256)
            assert R == resident_blocks(layers, cap), (layers, cap, R)
            assert nbytes == lds_bytes(layers, cap) <= LDS_LIMIT, (layers, cap, nbytes)
        assert resident_blocks(layers, 0) == 0 and resident_blocks(layers, 1) == 1
        assert resident_blocks(layers, 10 ** 6) == resident_blocks(layers)
    # what is resident: everything of a list lds16 serves; the front of the others
    assert resident_blocks([6, 48, 48, 4]) == stream_blocks([6, 48, 48, 4]) == 9 + 3 + AHEAD
    assert resident_blocks([6, 128, 128, 128, 4]) == stream_blocks([6, 128, 128, 128, 4])
    assert resident_blocks(W128x4) == (LDS_LIMIT - 16 * head_quads(W128x4)) // 1024 < stream_blocks(W128x4)
    big = [6, 256, 256, 4]
    assert stream_blocks(big) == 256 + 16 + AHEAD and resident_blocks(big) == 149 and lds_bytes(big) > LDS_LIMIT - 1024


def test_the_workgroup_rule(glb16_packer):
    wide, deep, small = [6, 256, 256, 4], W128x4, [6, 48, 48, 4]
    for layers, want in [(wide, {64: 256, 1920: 256, 16384: 256, 65536: 512}), (deep, {64: 256, 1920: 256, 16384: 256, 65536: 512}),
                         (small, {64: 256, 1920: 256, 16384: 256, 65536: 512}), ([6, 129, 4], {64: 256, 1920: 256, 16384: 256, 65536: 512})]:
        for K, threads in want.items():
            _, (_, _, got) = glb16_packer(layers, K=K, cus=256)
            assert got == workgroup_threads(layers, K, 256) == threads, (layers, K, got, workgroup_threads(layers, K, 256), threads)
    # a small LDS request leaves the registers to decide: two workgroups of 256 threads per CU, 32 768 rollouts on 256 CUs
    for K, threads in [(32768, 256), (32768 + 64, 512)]:
        _, (_, _, got) = glb16_packer(small, K=K, cus=256)
        assert got == workgroup_threads(small, K, 256) == threads, (K, got)
    # under "glb16_r0" the wide list asks for its head only
    _, (R, nbytes, got) = glb16_packer(wide, cap=0, K=32768, cus=256)
    assert (R, nbytes, got) == (0, 16 * head_quads(wide), 256) and got == workgroup_threads(wide, 32768, 256, cap=0)


def test_what_the_form_refuses(glb16_packer):
    """The basis-function model (no layer list), a list without a hidden layer, a hidden width above 256: no image, no LDS."""
    for layers in ([], [6, 4], [6, 257, 4], [6, 256, 257, 4], [6, 0, 4], [7, 16, 4], [6, 16, 5]):
        cap_line, (R, nbytes, threads) = glb16_packer(layers, K=1920, cus=256)
        assert cap_line[:4] == (0, 0, 0, 0) and (R, nbytes, threads) == (0, 0, 0), (layers, cap_line, R, nbytes, threads)
    assert glb16_packer([6, 256, 256, 256, 256, 256, 256, 4])[0][0] == 1
    assert glb16_packer([6, 1, 4])[0][0] == 1
