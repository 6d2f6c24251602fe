"""The LDS weight image of the "lds16" rollout form (csrc/abi_pack.hip: pack_lds16_weights; CPU only).

The packer, the capacity functions and the workgroup rule are ordinary functions of libmppi_hip.so; a small C++ program linked
against the library calls them (no export of the C ABI is involved).  The image, in float4 ("quads"); lane l = (row = l & 15,
kk = l >> 4), the neuron of row `row` of M tile m is n = 16 m + 4 (row & 3) + (row >> 2) (output layer: row & 3):
  biases   hidden weight layer j: 4 MT_j quads, quad 4 m + g = kTanhScale x (b[16 m + g], b[16 m + 4 + g], b[16 m + 8 + g],
           b[16 m + 12 + g]); then ONE quad b_out[0..3]
  layer 0  MT_0 half blocks of 32 quads: float2 l of half block m = (W[n][kk], W[n][4 + kk])
  layer j  blocks of 64 quads, quad l of block (m, mi) = (W[n][16 mi + 4 c + kk], c = 0..3): k-steps 4 mi .. 4 mi + 3 of tile m; the
           blocks in the order of their use: per pair P of tiles, per input tile mi, block (2 P, mi) then (2 P + 1, mi); then an odd
           last tile's blocks, mi ascending
  then 2 blocks of zeros.
Every weight is at its tile, row, k-step and lane, every bias at its slot, every other entry is exactly 0."""
import os
import subprocess

import numpy as np
import pytest

from autorally_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")
AHEAD = 2                                        # csrc/rollout_lds16.hip: kLds16Ahead (blocks)
TANH_SCALE = np.float32(2.88539008177792681472)  # csrc/mppi_device.hpp: kTanhScale
LDS_LIMIT = 160 * 1024

HARNESS = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace mppi {
struct NetDesc { int n_layers; int layers[8]; int max_width; int num_params; };
struct Lds16Net { int n_w; int img_f4; int mt[7]; int ks[7]; int off[7]; int boff[7]; int nout[7]; };
Lds16Net lds16_net_of(const NetDesc &net);
bool lds16_supported(const NetDesc &net);
int lds16_pack_floats(const NetDesc &net);
size_t lds16_lds_bytes(const NetDesc &net);
size_t lds16_lds_limit();
int lds16_block_threads(const NetDesc &net, int K, int cus);
}
namespace mppi_abi { std::vector<float> pack_lds16_weights(const std::vector<float> &theta, const mppi::NetDesc &net); }
int main(int argc, char **argv)
{
  mppi::NetDesc net{};
  net.n_layers = argc - 3;
  for (int i = 0; i < net.n_layers; i++) net.layers[i] = atoi(argv[3 + i]);
  for (int i = 0; i + 1 < net.n_layers; i++) net.num_params += (net.layers[i] + 1) * net.layers[i + 1];
  printf("%d %zu %zu\n", (int)mppi::lds16_supported(net), mppi::lds16_lds_bytes(net), mppi::lds16_lds_limit());
  if (argv[1][0] == '-') {  // the capacity answer only; "-K,cus": the workgroup too
    int K = 0, cus = 0;
    if (sscanf(argv[1], "-%d,%d", &K, &cus) == 2) printf("%d\n", mppi::lds16_block_threads(net, K, cus));
    return 0;
  }
  printf("%d\n", mppi::lds16_pack_floats(net));
  const mppi::Lds16Net d = mppi::lds16_net_of(net);
  printf("%d %d", d.n_w, d.img_f4);
  for (int j = 0; j < d.n_w; j++) printf(" %d %d %d %d %d", d.mt[j], d.ks[j], d.off[j], d.boff[j], d.nout[j]);
  printf("\n");
  std::vector<float> theta(net.num_params);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(theta.data(), 4, theta.size(), f) != theta.size()) return 2;
  fclose(f);
  const std::vector<float> img = mppi_abi::pack_lds16_weights(theta, net);
  f = fopen(argv[2], "wb");
  if (!f || fwrite(img.data(), 4, img.size(), f) != img.size()) return 3;
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    from autorally_amd import build as B
    B.build()
    d = tmp_path_factory.mktemp("lds16_pack")
    src, exe = str(d / "pack.cpp"), str(d / "pack")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(layers, theta=None, launch=None):
        """-> (supported, LDS bytes of a workgroup, the limit)[, threads per workgroup | pack floats, Lds16Net, image]"""
        tin, tout = str(d / "theta.bin"), str(d / "image.bin")
        if theta is not None:
            np.asarray(theta, np.float32).tofile(tin)
        first = tin if theta is not None else ("-%d,%d" % launch if launch else "-")
        r = subprocess.run([exe, first, tout] + [str(x) for x in layers], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        lines = r.stdout.split("\n")
        cap = tuple(int(x) for x in lines[0].split())
        if theta is None:
            return cap + (int(lines[1]),) if launch else cap
        return cap, int(lines[1]), [int(x) for x in lines[2].split()], np.fromfile(tout, np.float32)
    return run


def _tiles(layers):
    """MT per weight layer: ceil(nout / 16) for the hidden ones, 1 for the output layer"""
    return [(n + 15) // 16 for n in layers[1:-1]] + [1]


def image_quads(layers):
    mt = _tiles(layers)
    bias = 4 * sum(mt[:-1]) + 1
    return bias + 32 * mt[0] + 64 * sum(a * b for a, b in zip(mt[1:], mt[:-1])) + 64 * AHEAD


def _neuron(m, row, last):
    return (row & 3) if last else 16 * m + 4 * (row & 3) + (row >> 2)


def _block_index(m, mi, mt_out, mt_in):
    """where block (tile m, input tile mi) lies in its layer's stream"""
    if mt_out % 2 == 1 and m == mt_out - 1:
        return m * mt_in + mi
    return 2 * ((m // 2) * mt_in + mi) + (m % 2)


LISTS = [[6, 5, 7, 4], [6, 17, 4], [6, 16, 24, 4], [6, 65, 4], [6, 33, 97, 66, 4], [6, 128, 128, 4], [6, 128, 128, 128, 4]]


@pytest.mark.parametrize("layers", LISTS, ids=lambda l: "-".join(map(str, l)))
def test_every_weight_at_its_tile_row_kstep_and_lane_and_zeros_elsewhere(packer, layers):
    layers, theta = P.synthetic_model(layers, seed=9)
    theta = np.asarray(theta, np.float32)
    assert np.all(theta != 0.0)
    cap, floats, desc, img = packer(layers, theta)
    mt, n_w = _tiles(layers), len(layers) - 1
    assert img.size == floats == image_quads(layers) * 4
    assert cap == (1, img.size * 4, LDS_LIMIT) and cap[1] <= LDS_LIMIT, "the image is all of a workgroup's LDS"
    # Lds16Net: tiles, k-steps, offsets
    assert desc[:2] == [n_w, image_quads(layers)]
    per = [desc[2 + 5 * j:7 + 5 * j] for j in range(n_w)]
    boff, off = 0, 4 * sum(mt[:-1]) + 1
    for j in range(n_w):
        assert per[j] == [mt[j], 2 if j == 0 else 4 * mt[j - 1], off, boff, layers[j + 1]], (j, per[j])
        boff += 1 if j == n_w - 1 else 4 * mt[j]
        off += 32 * mt[0] if j == 0 else 64 * mt[j] * mt[j - 1]
    assert off + 64 * AHEAD == image_quads(layers)
    img = img.reshape(-1, 4)  # [quad][component]
    want = np.zeros_like(img)
    toff = 0
    for j, (nin, nout) in enumerate(zip(layers[:-1], layers[1:])):
        W = theta[toff:toff + nin * nout].reshape(nout, nin)
        b = theta[toff + nin * nout:toff + nin * nout + nout]
        last = j == n_w - 1
        _, _, woff, bo, _ = per[j]
        if last:
            want[bo] = b
        else:
            for m in range(mt[j]):
                for g in range(4):
                    for r in range(4):
                        if 16 * m + 4 * r + g < nout:
                            want[bo + 4 * m + g, r] = b[16 * m + 4 * r + g] * TANH_SCALE
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
                    for c in range(4):  # k-step 4 mi + c, k-slot kk
                        if 16 * mi + 4 * c + kk < nin:
                            want[blk + lane, c] = W[n, 16 * mi + 4 * c + kk]
        toff += nin * nout + nout
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    # said once more without the loop above
    # hidden biases times kTanhScale, each exactly once, register r of row group g of tile m = neuron 16 m + 4 r + g
    toff = 0
    for j, (nin, nout) in enumerate(zip(layers[:-2], layers[1:-1])):
        b = theta[toff + nin * nout:toff + nin * nout + nout] * TANH_SCALE
        quads = img[per[j][3]:per[j][3] + 4 * mt[j]].reshape(mt[j], 4, 4)  # [m][g][r]
        by_neuron = quads.transpose(0, 2, 1).reshape(-1)                   # 16 m + 4 r + g
        np.testing.assert_array_equal(by_neuron[:nout], b)
        assert not np.any(by_neuron[nout:])
        toff += nin * nout + nout
    np.testing.assert_array_equal(img[per[-1][3]], theta[-4:])
    # the first weights of layer 0: lane 0 (row 0, k-slot 0) of tile 0 holds W1[0][0], W1[0][4]; lane 17 (row 1, k-slot 1): neuron 4
    l0 = img[per[0][2]:per[0][2] + 32].reshape(64, 2)
    np.testing.assert_array_equal(l0[0], theta[[0, 4]])
    if layers[1] > 4:
        np.testing.assert_array_equal(l0[17], theta[[4 * 6 + 1, 4 * 6 + 5]])
    np.testing.assert_array_equal(l0[32:, 1], np.zeros(32, np.float32))  # k = 6, 7 do not exist
    # the output layer: one tile, rows 4 g' + o all hold output o; its first block, lane (row, kk), component c = W_out[row & 3][4 c + kk]
    W_out = theta[-(layers[-2] + 1) * 4:-4].reshape(4, layers[-2])
    out0 = img[per[-1][2]:per[-1][2] + 64]
    for lane in (0, 5, 22, 63):
        for c in range(4):
            k = 4 * c + (lane >> 4)
            assert out0[lane, c] == (W_out[lane & 3, k] if k < layers[-2] else 0.0)
    assert not np.any(img[-64 * AHEAD:])
    # every weight of the hidden layers once, the output layer's four times (rows 4 g' + o), 4 + hidden biases
    hidden = sum((nin + 1) * nout for nin, nout in zip(layers[:-2], layers[1:-1]))
    assert int(np.count_nonzero(img)) == hidden + 4 * 4 * layers[-2] + 4


def test_what_fits_one_workgroup(packer):
    """6-128-128-128-4 fits the 160 KB of a workgroup (about 142 KB of operands), one more 128-wide layer does not (its byte count
    is reported: the refusal states it); a hidden width above 128 and a list without a hidden layer are no lists of this form."""
    ok, nbytes, limit = packer([6, 128, 128, 128, 4])
    assert (ok, limit) == (1, LDS_LIMIT) and nbytes == image_quads([6, 128, 128, 128, 4]) * 16
    assert (4 + 64 + 64 + 8) * 1024 < nbytes < 148 * 1024
    ok, nbytes, limit = packer([6, 128, 128, 128, 128, 4])
    assert ok == 0 and nbytes == image_quads([6, 128, 128, 128, 128, 4]) * 16 and nbytes > LDS_LIMIT
    assert packer([6, 129, 4])[:2] == (0, 0)
    assert packer([6, 4])[:2] == (0, 0)
    assert packer([6, 64, 64, 64, 64, 64, 64, 4])[0] == 1
    assert packer([6, 1, 4])[0] == 1


def workgroup_threads(layers, K, cus):
    """The workgroup rule of csrc/rollout_lds16.hip (lds16_block_threads), said again: the smallest of 256 / 512 / 1024 threads for
    which every workgroup is resident at once -- floor(limit / image) workgroups per CU by the LDS, the instance's waves per SIMD
    (4 up to 64 wide, 3 beyond) by the registers -- else the largest the instance has (1024; 512 for the lists beyond 64 wide)."""
    wide = max(layers[1:-1]) > 64
    waves, wps, largest = K // 16, 3 if wide else 4, 512 if wide else 1024
    by_lds = LDS_LIMIT // (image_quads(layers) * 16)
    for threads in (256, 512, 1024):
        if threads > largest:
            break
        wpb = threads // 64
        if -(-waves // wpb) <= min(by_lds, 4 * wps // wpb) * cus:
            return threads
    return largest


def test_the_workgroup_rule(packer):
    big, mid, small = [6, 128, 128, 128, 4], [6, 64, 64, 64, 64, 64, 64, 4], [6, 48, 48, 4]
    for layers, K, cus, want in [(big, 16384, 256, 256), (big, 16384 + 64, 256, 512), (big, 32768, 256, 512), (big, 65536, 256, 512),
                                 (mid, 16384, 256, 256), (mid, 32768, 256, 512), (mid, 65536, 256, 1024), (mid, 65536 + 64, 256, 1024),
                                 (small, 16384, 256, 256), (small, 65536, 256, 256), (small, 65536 + 64, 256, 1024),
                                 (small, 1 << 18, 256, 1024), (small, 1984, 256, 256), (big, 1984, 8, 512), (small, 64, 1, 256)]:
        got = packer(layers, launch=(K, cus))[3]
        assert got == workgroup_threads(layers, K, cus) == want, (layers, K, cus, got, workgroup_threads(layers, K, cus), want)
