"""The LDS weight image of the "lds44" rollout form (csrc/abi_pack.hip: pack_lds44_weights; CPU only).

The packer is an ordinary function of libmppi_hip.so; a small C++ program linked against the library calls it (no export of the
C ABI is involved).  For a layer list whose widths are not multiples of four and for the largest one: every weight lands at
its lane and k, every bias at its lane (hidden ones times kTanhScale), every other entry is exactly 0, and the rows of the
output layer sit at lanes 0, 16, 32, 48."""
import os
import subprocess

import numpy as np
import pytest

from autorally_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")
BIAS_QUADS, AHEAD = 2, 3                       # csrc/mppi_kernels.hpp: kLds44BiasQuads, kLds44Ahead
TANH_SCALE = np.float32(2.88539008177792681472)  # csrc/mppi_device.hpp: kTanhScale

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace mppi { struct NetDesc { int n_layers; int layers[8]; int max_width; int num_params; }; }
namespace mppi_abi { std::vector<float> pack_lds44_weights(const std::vector<float> &theta, const mppi::NetDesc &net); }
int main(int argc, char **argv)
{
  mppi::NetDesc net{};
  net.n_layers = argc - 3;
  for (int i = 0; i < net.n_layers; i++) net.layers[i] = atoi(argv[3 + i]);
  for (int i = 0; i + 1 < net.n_layers; i++) net.num_params += (net.layers[i] + 1) * net.layers[i + 1];
  std::vector<float> theta(net.num_params);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(theta.data(), 4, theta.size(), f) != theta.size()) return 2;
  fclose(f);
  const std::vector<float> img = mppi_abi::pack_lds44_weights(theta, net);
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
    d = tmp_path_factory.mktemp("lds44_pack")
    src, exe = str(d / "pack.cpp"), str(d / "pack")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(layers, theta):
        tin, tout = str(d / "theta.bin"), str(d / "image.bin")
        np.asarray(theta, np.float32).tofile(tin)
        r = subprocess.run([exe, tin, tout] + [str(x) for x in layers], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return np.fromfile(tout, np.float32)
    return run


@pytest.mark.parametrize("layers", [[6, 5, 7, 4], [6, 64, 64, 64, 64, 64, 64, 4]], ids=lambda l: "-".join(map(str, l)))
def test_every_weight_at_its_lane_and_k_and_zeros_elsewhere(packer, layers):
    layers, theta = P.synthetic_model(layers, seed=9)
    theta = np.asarray(theta, np.float32)
    assert np.all(theta != 0.0)
    img = packer(layers, theta)
    quads = [(n + 3) // 4 for n in layers[:-1]]
    assert img.size == (BIAS_QUADS + sum(quads) + AHEAD) * 64 * 4
    img = img.reshape(-1, 64, 4)  # [quad][lane][component]
    want = np.zeros_like(img)
    off, q0, n_w = 0, BIAS_QUADS, len(layers) - 1
    for j, (nin, nout) in enumerate(zip(layers[:-1], layers[1:])):
        W = theta[off:off + nin * nout].reshape(nout, nin)
        b = theta[off + nin * nout:off + nin * nout + nout]
        last = j == n_w - 1
        for lane in range(64):
            n = (lane // 16 if lane % 16 == 0 else -1) if last else (lane if lane < nout else -1)
            want[j // 4, lane, j % 4] = b[lane // 16] if last else (b[n] * TANH_SCALE if n >= 0 else 0.0)
            if n >= 0:
                for k in range(nin):
                    want[q0 + k // 4, lane, k % 4] = W[n, k]
        q0 += quads[j]
        off += nin * nout + nout
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    # said once more without the loop above: the output rows at lanes 0, 16, 32, 48, nothing on the other lanes of that layer
    qo = BIAS_QUADS + sum(quads[:-1])
    out_rows = img[qo:qo + quads[-1]]
    W_out = theta[-(layers[-2] + 1) * 4:-4].reshape(4, layers[-2])
    for c in range(4):
        np.testing.assert_array_equal(out_rows[:, 16 * c, :].reshape(-1)[:layers[-2]], W_out[c])
    others = [lane for lane in range(64) if lane % 16]
    assert not np.any(out_rows[:, others, :]) and not np.any(img[-AHEAD:])
    assert int(np.count_nonzero(img)) == sum((nin + 1) * nout for nin, nout in zip(layers[:-2], layers[1:-1])) + 4 * layers[-2] + 64
