"""The register image of the "row32" / "row32_tree" rollout forms (csrc/abi_pack.hip: pack_row32_weights; CPU only).

The packer is an ordinary function of libmppi_hip.so; a small C++ program linked against the library calls it (no export of the
C ABI is involved; the pattern of tests/test_lds44_pack.py).  The image serves both forms: the exact output layer's entries and
the tree's three sit side by side, as in pack_row_weights' image.  For lists narrower than 32, of one hidden layer, of three and
of four: every weight and bias lands at its entry and lane (hidden biases times kTanhScale) and every other float is exactly 0;
for 6-32-32-4 the image is pack_row_weights' float for float, which is what hands the kernel the same registers."""
import os
import subprocess

import numpy as np
import pytest

from autorally_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")
TANH_SCALE = np.float32(2.88539008177792681472)  # csrc/mppi_device.hpp: kTanhScale
H = 32

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
namespace mppi { struct NetDesc { int n_layers; int layers[8]; int max_width; int num_params; }; }
namespace mppi_abi {
std::vector<float> pack_row32_weights(const std::vector<float> &theta, const mppi::NetDesc &net);
std::vector<float> pack_row_weights(const std::vector<float> &theta);
}
int main(int argc, char **argv)
{
  const bool row = strcmp(argv[1], "row") == 0;  // pack_row_weights (6-32-32-4 only)
  mppi::NetDesc net{};
  net.n_layers = argc - 4;
  for (int i = 0; i < net.n_layers; i++) net.layers[i] = atoi(argv[4 + i]);
  for (int i = 0; i + 1 < net.n_layers; i++) net.num_params += (net.layers[i] + 1) * net.layers[i + 1];
  std::vector<float> theta(net.num_params);
  FILE *f = fopen(argv[2], "rb");
  if (!f || fread(theta.data(), 4, theta.size(), f) != theta.size()) return 2;
  fclose(f);
  const std::vector<float> img = row ? mppi_abi::pack_row_weights(theta) : mppi_abi::pack_row32_weights(theta, net);
  f = fopen(argv[3], "wb");
  if (!f || fwrite(img.data(), 4, img.size(), f) != img.size()) return 3;
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    from autorally_amd import build as B
    B.build()
    d = tmp_path_factory.mktemp("row32_pack")
    src, exe = str(d / "pack.cpp"), str(d / "pack")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(which, layers, theta):
        tin, tout = str(d / "theta.bin"), str(d / "image.bin")
        np.asarray(theta, np.float32).tofile(tin)
        r = subprocess.run([exe, which, tin, tout] + [str(x) for x in layers], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return np.fromfile(tout, np.float32)
    return run


def _split(layers, theta):
    Ws, bs, off = [], [], 0
    for nin, nout in zip(layers[:-1], layers[1:]):
        Ws.append(theta[off:off + nin * nout].reshape(nout, nin))
        bs.append(theta[off + nin * nout:off + nin * nout + nout])
        off += nin * nout + nout
    return Ws, bs


def _layout(nhh):
    """csrc/mppi_kernels.hpp: row_pack_layout -- first entries of w2, w3, hidden biases, b3, tree; number of entries."""
    w3 = 3 + 16 * nhh
    bias = w3 + 16
    b3 = bias + (nhh + 2) // 2
    return 3, w3, bias, b3, b3 + 1, b3 + 4


def _expected(layers, theta):
    """[entry][lane p][4], written from the statement of the layout: lane p owns neurons 2p, 2p+1 of every hidden layer, outputs
    2(p&1), 2(p&1)+1 of the exact output layer, and its quad's output p >> 2 of the tree."""
    Ws, bs = _split(layers, theta)
    NH = len(layers) - 2
    e_w2, e_w3, e_bias, e_b3, e_tree, n = _layout(NH - 1)
    want = np.zeros((n, 16, 4), np.float32)
    placed = 0

    def w(l, nrn, k):
        nonlocal placed
        if nrn < layers[l + 1] and k < layers[l]:
            placed += 1
            return Ws[l][nrn, k]
        return np.float32(0)

    def b(l, nrn, scale):
        nonlocal placed
        if nrn < layers[l + 1]:
            placed += 1
            return np.float32(bs[l][nrn] * scale)
        return np.float32(0)
    one = np.float32(1)
    for p in range(16):
        j = (2 * p, 2 * p + 1)
        o = (2 * (p & 1), 2 * (p & 1) + 1)
        for k in range(6):
            for c in range(2):
                want[k // 2, p, 2 * (k & 1) + c] = w(0, j[c], k)
        for k in range(H):
            for l in range(1, NH):
                for c in range(2):
                    want[e_w2 + 16 * (l - 1) + k // 2, p, 2 * (k & 1) + c] = w(l, j[c], k)
            for c in range(2):
                want[e_w3 + k // 2, p, 2 * (k & 1) + c] = w(NH, o[c], k)
        for l in range(NH):
            for c in range(2):
                want[e_bias + l // 2, p, 2 * (l & 1) + c] = b(l, j[c], TANH_SCALE)
        for c in range(2):
            want[e_b3, p, c] = b(NH, o[c], one)
        q = p >> 2
        for i in range(4):  # output q ^ i at position i: (q, q^1) in the first tree entry, (q^2, q^3) in the second
            for c in range(2):
                want[e_tree + i // 2, p, 2 * c + (i & 1)] = w(NH, q ^ i, j[c])
        want[e_tree + 2, p, 0] = b(NH, q, one)
    return want, placed


LISTS = [[6, 5, 7, 4], [6, 9, 4], [6, 32, 32, 32, 4], [6, 32, 32, 32, 32, 4]]


@pytest.mark.parametrize("layers", LISTS, ids=lambda l: "-".join(map(str, l)))
def test_every_weight_at_its_entry_and_lane_and_zeros_elsewhere(packer, layers):
    layers, theta = P.synthetic_model(layers, seed=9)
    theta = np.asarray(theta, np.float32)
    assert np.all(theta != 0.0)
    img = packer("row32", layers, theta)
    NH = len(layers) - 2
    n = _layout(NH - 1)[5]
    assert img.size == n * 16 * 4
    img = img.reshape(n, 16, 4)
    want, placed = _expected(layers, theta)
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    # counted without the table above.  Per rollout (16 lanes): every hidden weight and bias once; the exact output layer's weights
    # and biases on 8 lanes each (every even / odd lane holds the same two outputs); the tree's weights once and its bias per quad
    hidden = sum((nin + 1) * nout for nin, nout in zip(layers[:-2], layers[1:-1]))
    count = hidden + 8 * 4 * layers[-2] + 8 * 4 + 4 * layers[-2] + 16
    assert placed == count and int(np.count_nonzero(img)) == count, (placed, count, int(np.count_nonzero(img)))
    # the hidden biases carry kTanhScale, b3 does not (said once more without the table)
    Ws, bs = _split(layers, theta)
    e_bias, e_b3 = _layout(NH - 1)[2:4]
    np.testing.assert_array_equal(img[e_bias, :(layers[1] + 1) // 2, 0], (bs[0] * TANH_SCALE)[0::2])
    np.testing.assert_array_equal(img[e_b3, 0, :2], bs[NH][:2])
    np.testing.assert_array_equal(img[e_b3, 1, :2], bs[NH][2:])


def test_the_image_of_6_32_32_4_is_the_row_forms(packer):
    """row_load<NHH = 1> reads pack_row_weights' entries (rollout_row.hip's kernels serve the two-layer lists): equal images are
    equal registers."""
    layers, theta = P.synthetic_model([6, 32, 32, 4], seed=4)
    theta = np.asarray(theta, np.float32)
    a, b = packer("row32", layers, theta), packer("row", layers, theta)
    assert a.size == 40 * 16 * 4
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    want, _ = _expected(layers, theta)
    np.testing.assert_array_equal(a.reshape(40, 16, 4).view(np.uint32), want.view(np.uint32))
