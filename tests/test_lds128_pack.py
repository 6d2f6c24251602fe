"""The LDS weight image of the "lds128" rollout form (csrc/abi_pack.hip: pack_lds128_weights; CPU only).

The packer and the capacity functions are ordinary functions of libmppi_hip.so; a small C++ program linked against the library
calls them (no export of the C ABI is involved).  The image: float4 q of lane l at float4 index q * 64 + l; 4 bias quads -- float
e = 2 j + h of lane l is the bias of neuron 64 h + l of weight layer j (hidden: times kTanhScale; the output layer at e = 2 j:
b_out[l >> 4]); then per weight layer ceil(nin / 4) x H quads, H = ceil(nout / 64) halves (1 for the output layer), INTERLEAVED:
quad q' H + h of the layer is (W[64 h + l][4 q'] .. W[64 h + l][4 q' + 3]), the output layer's row c at lane 16 c; then
kLds44Ahead quads of zeros.  For lists with one half, with two, with a partial quad behind the half boundary and for the
largest one: every weight is at its half, lane and k, every bias at its slot, every other entry is exactly 0."""
import os
import subprocess

import numpy as np
import pytest

from autorally_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")
BIAS_QUADS, AHEAD = 4, 3                       # csrc/mppi_kernels.hpp: kLds128BiasQuads, kLds44Ahead
TANH_SCALE = np.float32(2.88539008177792681472)  # csrc/mppi_device.hpp: kTanhScale
LDS_LIMIT = 160 * 1024

HARNESS = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace mppi {
struct NetDesc { int n_layers; int layers[8]; int max_width; int num_params; };
bool lds128_supported(const NetDesc &net);
int lds128_pack_floats(const NetDesc &net);
size_t lds128_lds_bytes(const NetDesc &net);
size_t lds128_lds_limit();
}
namespace mppi_abi { std::vector<float> pack_lds128_weights(const std::vector<float> &theta, const mppi::NetDesc &net); }
int main(int argc, char **argv)
{
  mppi::NetDesc net{};
  net.n_layers = argc - 3;
  for (int i = 0; i < net.n_layers; i++) net.layers[i] = atoi(argv[3 + i]);
  for (int i = 0; i + 1 < net.n_layers; i++) net.num_params += (net.layers[i] + 1) * net.layers[i + 1];
  printf("%d %zu %zu\n", (int)mppi::lds128_supported(net), mppi::lds128_lds_bytes(net), mppi::lds128_lds_limit());
  if (argv[1][0] == '-') return 0;  // the capacity answer only
  printf("%d\n", mppi::lds128_pack_floats(net));
  std::vector<float> theta(net.num_params);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(theta.data(), 4, theta.size(), f) != theta.size()) return 2;
  fclose(f);
  const std::vector<float> img = mppi_abi::pack_lds128_weights(theta, net);
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
    d = tmp_path_factory.mktemp("lds128_pack")
    src, exe = str(d / "pack.cpp"), str(d / "pack")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(layers, theta=None):
        """-> (supported, LDS bytes of a group, the limit)[, pack floats, image]"""
        tin, tout = str(d / "theta.bin"), str(d / "image.bin")
        if theta is not None:
            np.asarray(theta, np.float32).tofile(tin)
        r = subprocess.run([exe, tin if theta is not None else "-", tout] + [str(x) for x in layers], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        lines = r.stdout.split("\n")
        cap = tuple(int(x) for x in lines[0].split())
        if theta is None:
            return cap
        return cap, int(lines[1]), np.fromfile(tout, np.float32)
    return run


def _halves(layers):
    """H per weight layer: ceil(nout / 64) for the hidden ones, 1 for the output layer"""
    return [(n + 63) // 64 for n in layers[1:-1]] + [1]


def _image_quads(layers):
    return BIAS_QUADS + sum(((nin + 3) // 4) * H for nin, H in zip(layers[:-1], _halves(layers))) + AHEAD


@pytest.mark.parametrize("layers", [[6, 5, 7, 4], [6, 65, 4], [6, 33, 97, 66, 4], [6, 128, 128, 4]], ids=lambda l: "-".join(map(str, l)))
def test_every_weight_at_its_half_lane_and_k_and_zeros_elsewhere(packer, layers):
    layers, theta = P.synthetic_model(layers, seed=9)
    theta = np.asarray(theta, np.float32)
    assert np.all(theta != 0.0)
    cap, floats, img = packer(layers, theta)
    halves = _halves(layers)
    quads = [(n + 3) // 4 for n in layers[:-1]]
    assert img.size == floats == _image_quads(layers) * 64 * 4
    img = img.reshape(-1, 64, 4)  # [quad][lane][component]
    assert cap[0] == 1 and cap[2] == LDS_LIMIT and cap[1] <= LDS_LIMIT
    assert cap[1] - img.size * 4 in range(30 * 1024, 40 * 1024), "the group's rings in front of the image"
    want = np.zeros_like(img)
    off, q0, n_w = 0, BIAS_QUADS, len(layers) - 1
    for j, (nin, nout) in enumerate(zip(layers[:-1], layers[1:])):
        W = theta[off:off + nin * nout].reshape(nout, nin)
        b = theta[off + nin * nout:off + nin * nout + nout]
        last, H = j == n_w - 1, halves[j]
        for h in range(H):
            e = 2 * j + h
            for lane in range(64):
                n = (lane // 16 if lane % 16 == 0 else -1) if last else (64 * h + lane if 64 * h + lane < nout else -1)
                want[e // 4, lane, e % 4] = b[lane // 16] if last else (b[n] * TANH_SCALE if n >= 0 else 0.0)
                if n >= 0:
                    for k in range(nin):
                        want[q0 + (k // 4) * H + h, lane, k % 4] = W[n, k]
        q0 += quads[j] * H
        off += nin * nout + nout
    assert q0 + AHEAD == img.shape[0]
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    # said once more without the loop above.  Hidden biases times kTanhScale at float 2 j + h, lane = neuron - 64 h
    off = 0
    for j, (nin, nout) in enumerate(zip(layers[:-2], layers[1:-1])):
        b = theta[off + nin * nout:off + nin * nout + nout] * TANH_SCALE
        slots = np.concatenate([img[(2 * j + h) // 4, :, (2 * j + h) % 4] for h in range(2)])
        np.testing.assert_array_equal(slots[:nout], b)
        assert not np.any(slots[nout:])  # neurons that do not exist; with one half, float 2 j + 1 is nobody's
        off += nin * nout + nout
    # the first weight of the second half: neuron 64 of the first hidden layer sits in quad 1 of layer 0, lane 0
    if layers[1] > 64:
        np.testing.assert_array_equal(img[BIAS_QUADS + 1, 0, :], theta[64 * 6:64 * 6 + 4])
        np.testing.assert_array_equal(img[BIAS_QUADS + 3, 0, :2], theta[64 * 6 + 4:64 * 6 + 6])
    # the output rows at lanes 0, 16, 32, 48, nothing on the other lanes of that layer
    qo = img.shape[0] - AHEAD - quads[-1]
    out_rows = img[qo:qo + quads[-1]]
    W_out = theta[-(layers[-2] + 1) * 4:-4].reshape(4, layers[-2])
    for c in range(4):
        np.testing.assert_array_equal(out_rows[:, 16 * c, :].reshape(-1)[:layers[-2]], W_out[c])
    others = [lane for lane in range(64) if lane % 16]
    assert not np.any(out_rows[:, others, :]) and not np.any(img[-AHEAD:])
    e_out = 2 * (n_w - 1)
    np.testing.assert_array_equal(img[e_out // 4, :, e_out % 4], np.repeat(theta[-4:], 16))
    assert int(np.count_nonzero(img)) == sum((nin + 1) * nout for nin, nout in zip(layers[:-2], layers[1:-1])) + 4 * layers[-2] + 64


def test_what_fits_one_group(packer):
    """6-128-128-4 fits the 160 KB of a group, 6-128-128-128-4 does not (its byte count is reported: the refusal states it); a
    hidden width above 128 and a list without a hidden layer are no lists of this form at all."""
    ok, nbytes, limit = packer([6, 128, 128, 4])
    assert (ok, limit) == (1, LDS_LIMIT) and _image_quads([6, 128, 128, 4]) * 1024 < nbytes <= LDS_LIMIT
    rings = nbytes - _image_quads([6, 128, 128, 4]) * 1024
    ok, nbytes, limit = packer([6, 128, 128, 128, 4])
    assert ok == 0 and nbytes == rings + _image_quads([6, 128, 128, 128, 4]) * 1024 and nbytes > LDS_LIMIT
    assert _image_quads([6, 128, 128, 128, 4]) * 1024 > LDS_LIMIT, "the image alone"
    assert packer([6, 129, 4])[:2] == (0, 0)
    assert packer([6, 4])[:2] == (0, 0)
    assert packer([6, 64, 64, 64, 64, 64, 64, 4])[0] == 1  # 64 wide at the most: accepted
