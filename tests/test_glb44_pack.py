"""The weight image and the residency rule of the "glb44" rollout form (csrc/rollout_glb44.hip, csrc/abi_pack.hip:
pack_glb44_weights; CPU only).

The packer and the rules are ordinary functions of libmppi_hip.so; a small C++ program linked against the library calls them (no
export of the C ABI is involved).  The element of the image is a 1 KB quad: float4 q of lane l at float4 index q * 64 + l.
  bias quads   BIAS_QUADS = 7 (one per weight layer): float h of quad j of lane l = bias of neuron 64 h + l of weight layer j --
               hidden layers x kTanhScale, 0 where the neuron does not exist; output layer, float 0: b_out[l >> 4]
  per layer    ceil(nin / 4) x H quads, H = ceil(nout / 64) halves (1 for the output layer), interleaved in the order of their
               use: quad q' H + h = W[64 h + l][4 q' .. 4 q' + 3]; the output layer's row c at lane 16 c
  then         AHEAD quads of zeros.
The HEAD (bias quads + layer 0) is always in LDS behind the group's shared state.  Of the stream behind it R quads are resident:
  R = min(stream quads with the zero quads, floor((160 KB - shared state - head bytes) / 1 KB), the cap of "glb44_r<N>")."""
import os
import subprocess

import numpy as np
import pytest

from autorally_amd import params as P
from tests.test_lds16_pack import LDS_LIMIT, TANH_SCALE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")
AHEAD = 8          # csrc/mppi_kernels.hpp: kGlb44Ahead (quads)
BIAS_QUADS = 7     # csrc/mppi_kernels.hpp: kGlb44BiasQuads
LDS128_BIAS_QUADS, LDS128_AHEAD = 4, 3  # kLds128BiasQuads, kLds44Ahead

HARNESS = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace mppi {
struct NetDesc { int n_layers; int layers[8]; int max_width; int num_params; };
bool glb44_supported(const NetDesc &net);
int glb44_pack_floats(const NetDesc &net);
size_t glb44_head_bytes(const NetDesc &net);
int glb44_stream_quads(const NetDesc &net);
int glb44_resident_quads(const NetDesc &net, int cap);
size_t glb44_lds_bytes(const NetDesc &net, int cap);
size_t glb44_lds_limit();
bool lds128_supported(const NetDesc &net);
size_t lds128_lds_bytes(const NetDesc &net);
int lds128_pack_floats(const NetDesc &net);
}
namespace mppi_abi {
std::vector<float> pack_glb44_weights(const std::vector<float> &theta, const mppi::NetDesc &net);
std::vector<float> pack_lds128_weights(const std::vector<float> &theta, const mppi::NetDesc &net);
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
  // argv: theta file | "-cap", image file, lds128 image file, layers...
  mppi::NetDesc net{};
  net.n_layers = argc - 4;
  for (int i = 0; i < net.n_layers; i++) net.layers[i] = atoi(argv[4 + i]);
  for (int i = 0; i + 1 < net.n_layers; i++) net.num_params += (net.layers[i] + 1) * net.layers[i + 1];
  printf("%d %d %zu %d %zu\n", (int)mppi::glb44_supported(net), mppi::glb44_pack_floats(net), mppi::glb44_head_bytes(net),
         mppi::glb44_stream_quads(net), mppi::glb44_lds_limit());
  if (argv[1][0] == '-') {  // the rule: R and the LDS bytes under a cap; the group's shared state in front of the image
    const int cap = atoi(argv[1] + 1);
    const size_t shared = mppi::lds128_lds_bytes(net) ? mppi::lds128_lds_bytes(net) - 4 * (size_t)mppi::lds128_pack_floats(net) : 0;
    printf("%d %zu %zu\n", mppi::glb44_resident_quads(net, cap), mppi::glb44_lds_bytes(net, cap), shared);
    return 0;
  }
  std::vector<float> theta(net.num_params);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(theta.data(), 4, theta.size(), f) != theta.size()) return 2;
  fclose(f);
  if (int rc = dump(argv[2], mppi_abi::pack_glb44_weights(theta, net))) return rc;
  return dump(argv[3], mppi::lds128_supported(net) ? mppi_abi::pack_lds128_weights(theta, net) : std::vector<float>());
}
"""


@pytest.fixture(scope="module")
def glb44_packer(tmp_path_factory):
    from autorally_amd import build as B
    B.build()
    d = tmp_path_factory.mktemp("glb44_pack")
    src, exe = str(d / "pack.cpp"), str(d / "pack")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG])

    def run(layers, theta=None, cap=-1):
        """-> (supported, pack floats, head bytes, stream quads, the limit), then
        without theta: (R, LDS bytes, bytes of the shared state lds128 puts in front of ITS image) under `cap`;
        with theta: the image, lds128's image (empty where that form does not serve the list)"""
        tin, tout, tout128 = str(d / "theta.bin"), str(d / "image.bin"), str(d / "image128.bin")
        if theta is not None:
            np.asarray(theta, np.float32).tofile(tin)
        first = tin if theta is not None else "-%d" % cap
        r = subprocess.run([exe, first, tout, tout128] + [str(x) for x in layers], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        lines = r.stdout.split("\n")
        cap_line = tuple(int(x) for x in lines[0].split())
        if theta is None:
            return cap_line, tuple(int(x) for x in lines[1].split())
        return cap_line, np.fromfile(tout, np.float32), np.fromfile(tout128, np.float32)
    return run


def halves(nout):
    return -(-nout // 64)


def layer_quads(layers):
    """per weight layer: ceil(nin / 4) x H quads (the output layer: H = 1)"""
    n_w = len(layers) - 1
    return [-(-layers[j] // 4) * (halves(layers[j + 1]) if j < n_w - 1 else 1) for j in range(n_w)]


def head_quads(layers):
    return BIAS_QUADS + 2 * halves(layers[1])


def stream_quads(layers):
    return sum(layer_quads(layers)[1:]) + AHEAD


def image_quads(layers):
    return head_quads(layers) + stream_quads(layers)


def resident_quads(layers, shared, cap=-1):
    r = min(stream_quads(layers), (LDS_LIMIT - shared - 1024 * head_quads(layers)) // 1024)
    return r if cap < 0 else min(r, cap)


def lds_bytes(layers, shared, cap=-1):
    return shared + 1024 * (head_quads(layers) + resident_quads(layers, shared, cap))


def expected_image(layers, theta):
    """every weight at its quad, lane and component, every bias at its slot, zeros elsewhere: [quad][lane][component]"""
    n_w = len(layers) - 1
    want = np.zeros((image_quads(layers), 64, 4), np.float32)
    q0, toff = BIAS_QUADS, 0
    for j, (nin, nout) in enumerate(zip(layers[:-1], layers[1:])):
        W = theta[toff:toff + nin * nout].reshape(nout, nin)
        b = theta[toff + nin * nout:toff + nin * nout + nout]
        last = j == n_w - 1
        H = 1 if last else halves(nout)
        for lane in range(64):
            if last:
                want[j, lane, 0] = b[lane >> 4]
                rows = [(0, lane >> 4)] if lane % 16 == 0 else []
            else:
                rows = [(h, 64 * h + lane) for h in range(H) if 64 * h + lane < nout]
            for h, n in rows:
                if not last:
                    want[j, lane, h] = b[n] * TANH_SCALE
                for k in range(nin):
                    want[q0 + (k // 4) * H + h, lane, k % 4] = W[n, k]
        q0 += -(-nin // 4) * H
        toff += nin * nout + nout
    assert q0 + AHEAD == image_quads(layers)
    return want


DEEP8 = [6, 20, 70, 9, 130, 33, 65, 4]
LISTS = [[6, 65, 4], [6, 129, 4], [6, 193, 4], [6, 129, 193, 4], [6, 256, 7, 4], [6, 128, 128, 128, 4], DEEP8]


@pytest.mark.parametrize("layers", LISTS, ids=lambda l: "-".join(map(str, l)))
def test_every_weight_at_its_quad_lane_and_component_and_zeros_elsewhere(glb44_packer, layers):
    layers, theta = P.synthetic_model(layers, seed=9)
    theta = np.asarray(theta, np.float32)
    assert np.all(theta != 0.0)
    cap, img, _ = glb44_packer(layers, theta)
    assert cap == (1, image_quads(layers) * 256, head_quads(layers) * 1024, stream_quads(layers), LDS_LIMIT), cap
    assert img.size == image_quads(layers) * 256
    want = expected_image(layers, theta)
    img = img.reshape(-1, 64, 4)
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    assert not np.any(img[-AHEAD:])
    # every weight and bias of the hidden layers once, the output layer's weights once, its biases at every 16 lanes of a row
    hidden = sum((nin + 1) * nout for nin, nout in zip(layers[:-2], layers[1:-1]))
    assert int(np.count_nonzero(img)) == hidden + 4 * layers[-2] + 64


@pytest.mark.parametrize("layers", [[6, 33, 97, 66, 4], [6, 128, 128, 4]], ids=lambda l: "-".join(map(str, l)))
def test_the_weight_stream_is_lds128s(glb44_packer, layers):
    """Behind the bias quads the weights are pack_lds128_weights' float for float; the biases are the same numbers at (j, h)."""
    layers, theta = P.synthetic_model(layers, seed=10)
    _, img, img128 = glb44_packer(layers, np.asarray(theta, np.float32))
    n = 256 * sum(layer_quads(layers))
    assert img128.size == 256 * (LDS128_BIAS_QUADS + LDS128_AHEAD) + n and img.size == 256 * (BIAS_QUADS + AHEAD) + n
    a, b = img[256 * BIAS_QUADS:256 * BIAS_QUADS + n], img128[256 * LDS128_BIAS_QUADS:256 * LDS128_BIAS_QUADS + n]
    assert np.count_nonzero(a) > n // 4
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    bq, bq128 = img[:256 * BIAS_QUADS].reshape(BIAS_QUADS, 64, 4), img128[:256 * LDS128_BIAS_QUADS].reshape(-1, 64, 4)
    for j in range(len(layers) - 1):
        for h in range(2):
            e = 2 * j + h
            np.testing.assert_array_equal(bq[j, :, h].view(np.uint32), bq128[e >> 2, :, e & 3].view(np.uint32))
    assert not np.any(bq[:, :, 2:])


def test_the_residency_rule(glb44_packer):
    """Head bytes, R without a cap, under cap 0, cap 1 and a cap beyond capacity; the request never passes 160 KB."""
    _, (_, _, shared) = glb44_packer([6, 16, 4])
    assert 0 < shared <= 40 * 1024 and shared % 16 == 0, shared  # m44_group.hpp: M44GroupShared (the record rings)
    W128x4, W256x6 = [6, 128, 128, 128, 128, 4], [6, 256, 256, 256, 256, 256, 256, 4]
    for layers in LISTS + [W128x4, W256x6, [6, 1, 4], [6, 200, 256, 4], [6, 256, 256, 4], [6, 33, 97, 66, 4]]:
        cap_line, _ = glb44_packer(layers)
        assert cap_line[2] == 1024 * head_quads(layers) <= 15 * 1024, (layers, cap_line)
        for cap in (-1, 0, 1, 10 ** 6):
            _, (R, nbytes, _) = glb44_packer(layers, cap=cap)
            assert R == resident_quads(layers, shared, cap), (layers, cap, R)
            assert nbytes == lds_bytes(layers, shared, cap) <= LDS_LIMIT, (layers, cap, nbytes)
        assert resident_quads(layers, shared, 0) == 0 and resident_quads(layers, shared, 1) == 1
        assert resident_quads(layers, shared, 10 ** 6) == resident_quads(layers, shared)
    # what is resident: everything of a list lds128 serves; the front of the others
    assert resident_quads([6, 33, 97, 66, 4], shared) == stream_quads([6, 33, 97, 66, 4]) == 9 * 2 + 25 * 2 + 17 + AHEAD
    full = (LDS_LIMIT - shared) // 1024  # quads behind the shared state
    for layers in ([6, 128, 128, 128, 4], W128x4, [6, 256, 256, 4], W256x6):
        assert resident_quads(layers, shared) == full - head_quads(layers) < stream_quads(layers), layers
    assert stream_quads([6, 128, 128, 128, 4]) == 64 + 64 + 32 + AHEAD and stream_quads([6, 256, 256, 4]) == 256 + 64 + AHEAD


def test_what_the_form_refuses(glb44_packer):
    """The basis-function model (no layer list), a list without a hidden layer, a hidden width above 256: no image, no LDS."""
    for layers in ([], [6, 4], [6, 257, 4], [6, 256, 257, 4], [6, 0, 4], [7, 16, 4], [6, 16, 5]):
        cap_line, (R, nbytes, _) = glb44_packer(layers)
        assert cap_line[:4] == (0, 0, 0, 0) and (R, nbytes) == (0, 0), (layers, cap_line, R, nbytes)
    assert glb44_packer([6, 256, 256, 256, 256, 256, 256, 4])[0][0] == 1
    assert glb44_packer([6, 1, 4])[0][0] == 1
