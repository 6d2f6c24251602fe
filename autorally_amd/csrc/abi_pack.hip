// abi_pack.hip -- register / LDS images of the network weights for every kernel form, and the MRG32k3a jump tables.
#include "abi_internal.hpp"

using namespace mppi;
using namespace mppi_abi;

namespace mppi_abi {

constexpr uint64_t M1 = 4294967087ULL, M2 = 4294944443ULL;

struct Mat3 {
  uint32_t a[9];
};
Mat3 mat_mul(const Mat3 &A, const Mat3 &B, uint64_t m)
{
  Mat3 R;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      uint64_t acc = 0;
      for (int k = 0; k < 3; k++) acc = (acc + (uint64_t)A.a[3 * i + k] * B.a[3 * k + j] % m) % m;
      R.a[3 * i + j] = (uint32_t)acc;
    }
  return R;
}
Mat3 mat_identity()
{
  Mat3 R{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  return R;
}
Mat3 mat_pow(Mat3 A, uint64_t e, uint64_t m)
{
  Mat3 R = mat_identity();
  while (e) {
    if (e & 1) R = mat_mul(R, A, m);
    A = mat_mul(A, A, m);
    e >>= 1;
  }
  return R;
}
Mat3 base_A1() { return Mat3{{0, 1, 0, 0, 0, 1, (uint32_t)(M1 - 810728ULL), 1403580u, 0}}; }
Mat3 base_A2() { return Mat3{{0, 1, 0, 0, 0, 1, (uint32_t)(M2 - 1370589ULL), 0, 527612u}}; }

int compute_k99(int K)
{
  // smallest k with (double)k >= .99*NUM_ROLLOUTS, mppi_controller.cu:141
  const double thr = .99 * (double)K;
  int k = 0;
  while (k < K && !((double)k >= thr)) k++;
  return k;
}

// A-operand / bias register image for rollout_mfma.hip (see the mapping comment there).
std::vector<float> pack_mfma_weights(const std::vector<float> &theta, int H, int NHID)
{
  const int MT = H / 16, KSH = H / 4;
  const int nA0 = MT * 2, nAH = MT * KSH, nAL = KSH;
  const int nA = nA0 + (NHID - 1) * nAH + nAL;
  const int nBias = NHID * MT * 4 + 4;
  const int nTree = 4 * KSH + 1;  // mfma_net.hpp: MfmaTree -- the output layer for the butterfly form, behind the MFMA image
  std::vector<float> out((size_t)(nA + nBias + nTree) * 64, 0.0f);
  // offsets of W_l / b_l in theta, layers = 6, H x NHID, 4
  std::vector<int> wo, bo, nin, nout;
  int off = 0, prev = kNetIn;
  for (int l = 0; l <= NHID; l++) {
    const int no = (l < NHID) ? H : kNetOut;
    wo.push_back(off);
    bo.push_back(off + no * prev);
    nin.push_back(prev);
    nout.push_back(no);
    off += no * prev + no;
    prev = no;
  }
  for (int lane = 0; lane < 64; lane++) {
    const int row = lane & 15, kk = lane >> 4;  // A operand: A[row][k = kk]
    const int gq = row >> 2, rq = row & 3;
    // layer 0
    for (int m = 0; m < MT; m++)
      for (int s = 0; s < 2; s++) {
        const int n = 16 * m + 4 * rq + gq, kap = 4 * s + kk;
        out[(size_t)(m * 2 + s) * 64 + lane] = (kap < kNetIn) ? theta[wo[0] + n * kNetIn + kap] : 0.0f;
      }
    for (int l = 1; l < NHID; l++) {
      const int aoff = nA0 + (l - 1) * nAH;
      for (int m = 0; m < MT; m++)
        for (int s = 0; s < KSH; s++) {
          const int n = 16 * m + 4 * rq + gq, kap = 4 * s + kk;
          out[(size_t)(aoff + m * KSH + s) * 64 + lane] = theta[wo[l] + n * H + kap];
        }
    }
    {
      const int aoff = nA0 + (NHID - 1) * nAH;
      for (int s = 0; s < KSH; s++) {
        const int o = row & 3, kap = 4 * s + kk;
        out[(size_t)(aoff + s) * 64 + lane] = theta[wo[NHID] + o * H + kap];
      }
    }
    // biases: lane (j, g) register (m, r) holds D row 16m+4g+r = neuron 16m+4r+g
    const int g = lane >> 4;
    for (int l = 0; l < NHID; l++)
      for (int m = 0; m < MT; m++)
        for (int r = 0; r < 4; r++)
          out[(size_t)(nA + l * MT * 4 + m * 4 + r) * 64 + lane] = theta[bo[l] + 16 * m + 4 * r + g];
    for (int r = 0; r < 4; r++) out[(size_t)(nA + NHID * MT * 4 + r) * 64 + lane] = theta[bo[NHID] + r];
    // tree form of the output layer: lane (j, g) multiplies activation 4 s + g into outputs 0..3; its bias is b3[g]
    for (int s = 0; s < KSH; s++)
      for (int o = 0; o < 4; o++) out[(size_t)(nA + nBias + 4 * s + o) * 64 + lane] = theta[wo[NHID] + o * H + 4 * s + g];
    out[(size_t)(nA + nBias + 4 * KSH) * 64 + lane] = theta[bo[NHID] + g];
  }
  return out;
}

// Register image of the row form (rollout_row.hip: row_load): lane p of a rollout owns neurons 2p, 2p+1 of the hidden layers
// and outputs 2(p&1), 2(p&1)+1; entry i of lane p is float4 index i * 16 + p.  Hidden biases times kTanhScale.
std::vector<float> pack_row_weights(const std::vector<float> &theta)
{
  const int H = 32;
  const float *W1 = theta.data(), *B1 = W1 + H * kNetIn, *W2 = B1 + H, *B2 = W2 + H * H, *W3 = B2 + H, *B3 = W3 + kNetOut * H;
  std::vector<float> out((size_t)row_pack_floats(), 0.0f);
  for (int p = 0; p < 16; p++) {
    const int j0 = 2 * p, j1 = 2 * p + 1, o0 = 2 * (p & 1), o1 = o0 + 1;
    auto entry = [&](int i) { return &out[((size_t)i * 16 + p) * 4]; };
    for (int i = 0; i < 3; i++) {
      float *e = entry(i);
      e[0] = W1[j0 * kNetIn + 2 * i]; e[1] = W1[j1 * kNetIn + 2 * i];
      e[2] = W1[j0 * kNetIn + 2 * i + 1]; e[3] = W1[j1 * kNetIn + 2 * i + 1];
    }
    for (int i = 0; i < H / 2; i++) {
      float *e = entry(3 + i), *f = entry(3 + H / 2 + i);
      e[0] = W2[j0 * H + 2 * i]; e[1] = W2[j1 * H + 2 * i]; e[2] = W2[j0 * H + 2 * i + 1]; e[3] = W2[j1 * H + 2 * i + 1];
      f[0] = W3[o0 * H + 2 * i]; f[1] = W3[o1 * H + 2 * i]; f[2] = W3[o0 * H + 2 * i + 1]; f[3] = W3[o1 * H + 2 * i + 1];
    }
    float *b = entry(35), *c = entry(36);
    b[0] = B1[j0] * kTanhScale; b[1] = B1[j1] * kTanhScale; b[2] = B2[j0] * kTanhScale; b[3] = B2[j1] * kTanhScale;
    c[0] = B3[o0]; c[1] = B3[o1];
    // tree form (row_out_tree): this lane's own two activations into the four outputs, output (p >> 2) ^ i at position i
    const int o = p >> 2;
    float *t0 = entry(37), *t1 = entry(38), *t2 = entry(39);
    t0[0] = W3[o * H + j0]; t0[1] = W3[(o ^ 1) * H + j0]; t0[2] = W3[o * H + j1]; t0[3] = W3[(o ^ 1) * H + j1];
    t1[0] = W3[(o ^ 2) * H + j0]; t1[1] = W3[(o ^ 3) * H + j0]; t1[2] = W3[(o ^ 2) * H + j1]; t1[3] = W3[(o ^ 3) * H + j1];
    t2[0] = B3[o];
  }
  return out;
}

// Register image of the row form for a layer list of one to four hidden layers up to 32 wide (rollout_row32.hip; row_group.hpp:
// row_load<NHH>, NHH = hidden layers - 1): pack_row_weights' register order with 16 entries per hidden-to-hidden layer, at the
// entries of row_pack_layout(NHH) -- w1; the hidden-to-hidden layers; the exact output layer; the pre-scaled hidden biases, two
// layers per entry; b3; the tree's three entries.  A neuron or an input a layer does not have (width < 32) is weight 0, bias 0;
// every float that holds no weight or bias is exactly 0.  For 6-32-32-4 this is pack_row_weights' image float for float.
std::vector<float> pack_row32_weights(const std::vector<float> &theta, const NetDesc &net)
{
  std::vector<float> out((size_t)row32_pack_floats(net), 0.0f);
  if (out.empty()) return out;
  const int NH = net.n_layers - 2, H = 32;
  const RowPackLayout E = row_pack_layout(NH - 1);
  const float *Wl[8], *Bl[8];
  {
    const float *p = theta.data();
    for (int l = 0; l <= NH; l++) {
      Wl[l] = p;
      Bl[l] = p + (size_t)net.layers[l + 1] * net.layers[l];
      p += (size_t)net.layers[l + 1] * net.layers[l] + net.layers[l + 1];
    }
  }
  // weight (n, k) of weight layer l, bias n: 0 where the list has no such neuron or input
  auto w = [&](int l, int n, int k) { return (n < net.layers[l + 1] && k < net.layers[l]) ? Wl[l][(size_t)n * net.layers[l] + k] : 0.0f; };
  auto b = [&](int l, int n) { return n < net.layers[l + 1] ? Bl[l][n] : 0.0f; };
  for (int p = 0; p < 16; p++) {
    const int j0 = 2 * p, j1 = 2 * p + 1, o0 = 2 * (p & 1), o1 = o0 + 1;
    auto entry = [&](int i) { return &out[((size_t)i * 16 + p) * 4]; };
    for (int i = 0; i < 3; i++) {
      float *e = entry(i);
      e[0] = w(0, j0, 2 * i); e[1] = w(0, j1, 2 * i); e[2] = w(0, j0, 2 * i + 1); e[3] = w(0, j1, 2 * i + 1);
    }
    for (int i = 0; i < H / 2; i++) {
      for (int l = 1; l < NH; l++) {
        float *e = entry(E.w2 + (l - 1) * (H / 2) + i);
        e[0] = w(l, j0, 2 * i); e[1] = w(l, j1, 2 * i); e[2] = w(l, j0, 2 * i + 1); e[3] = w(l, j1, 2 * i + 1);
      }
      float *f = entry(E.w3 + i);
      f[0] = w(NH, o0, 2 * i); f[1] = w(NH, o1, 2 * i); f[2] = w(NH, o0, 2 * i + 1); f[3] = w(NH, o1, 2 * i + 1);
    }
    for (int l = 0; l < NH; l++) {
      float *e = entry(E.bias + l / 2) + 2 * (l & 1);
      e[0] = b(l, j0) * kTanhScale; e[1] = b(l, j1) * kTanhScale;
    }
    float *c = entry(E.b3);
    c[0] = b(NH, o0); c[1] = b(NH, o1);
    // tree form (row_out_tree): this lane's own two activations into the four outputs, output (p >> 2) ^ i at position i
    const int o = p >> 2;
    float *t0 = entry(E.tree), *t1 = entry(E.tree + 1), *t2 = entry(E.tree + 2);
    t0[0] = w(NH, o, j0); t0[1] = w(NH, o ^ 1, j0); t0[2] = w(NH, o, j1); t0[3] = w(NH, o ^ 1, j1);
    t1[0] = w(NH, o ^ 2, j0); t1[1] = w(NH, o ^ 3, j0); t1[2] = w(NH, o ^ 2, j1); t1[3] = w(NH, o ^ 3, j1);
    t2[0] = b(NH, o);
  }
  return out;
}

// Per-lane image of the basis-function row form (rollout_bf_row.hip: bf_row_load; the layout is written down at
// kBfRowSlots, mppi_kernels.hpp): lane p = 4 j + y of a rollout's DPP row runs y-thread y of output j, slot m of the lane is
// basis function i = y + 4 m.  The divisors are those of basis_funcs_from (basis_funcs.hpp; car_bfs.cuh:44-120), 0 = the basis
// function is its numerator; the reciprocals are the RN(1 / c) of MPPI_DIVC.
std::vector<float> pack_bf_row_weights(const std::vector<float> &W)
{
  static const float kDiv[kNumBfs] = {0.0f, 10.0f, 1200.0f, 1440000.0f, 1728000000.0f, 25.0f, 10.0f, 10.0f, 0.0f, 40.0f,
                                      1400.0f, 1960000.0f, 2744000000.0f, 40.0f, 1600.0f, 64000.0f, 50.0f, 0.0f, 0.0f, 3.0f,
                                      5.0f, 100.0f, 1000.0f, 0.0f, 0.0f};
  std::vector<float> out((size_t)bf_row_pack_floats(), 0.0f);
  for (int p = 0; p < 16; p++) {
    const int j = p >> 2, y = p & 3;
    auto slot = [&](int e0, int m) { return &out[((size_t)(e0 + m / 4) * 16 + p) * 4 + m % 4]; };
    unsigned marks = 0;
    for (int m = 0; m < kBfRowSlots; m++) {
      const int i = y + 4 * m;
      const bool used = i < kNumBfs, plain = !used || kDiv[i] == 0.0f;
      const float c = plain ? 1.0f : kDiv[i];
      *slot(0, m) = used ? W[(size_t)j * kNumBfs + i] : 0.0f;
      *slot(2, m) = c;
      *slot(4, m) = 1.0f / c;
      if (plain) marks |= kBfRowPlain << m;
      if (i == 9 || i == 13 || i == 14 || i == 15) marks |= kBfRowBigOnly << m;
      if (used) marks |= kBfRowUsed << m;
      if (i == 13 || i == 14) marks |= kBfRowDouble;
    }
    memcpy(slot(0, kBfRowSlots), &marks, sizeof(marks));  // the last word of entry 1
  }
  return out;
}

// Image of the 64-wide row form (rollout_row64.hip: row64_load + the LDS part): lane g of a 32-lane rollout owns neurons
// 2g, 2g+1 of every hidden layer; register entry i of lane g at float4 index i * 32 + g, then the 64 x 64 layers as
// [layer][k][g] pairs.  Hidden biases times kTanhScale.  Output layer in the order of row64_out_tree: Q = outputs {0, 1},
// P = outputs {2, 3}, inside each the output the lane keeps at the row_ror:8 level (bit 3 of g) first.
std::vector<float> pack_row64_weights(const std::vector<float> &theta, int NHID)
{
  const int H = 64, NB = (NHID + 1) / 2, NE = 3 + NB + 3;
  std::vector<float> out((size_t)row64_pack_floats(NHID), 0.0f);
  std::vector<const float *> Wl(NHID + 1), Bl(NHID + 1);
  {
    const float *p = theta.data();
    int prev = kNetIn;
    for (int l = 0; l <= NHID; l++) {
      const int no = (l < NHID) ? H : kNetOut;
      Wl[l] = p;
      Bl[l] = p + (size_t)no * prev;
      p += (size_t)no * prev + no;
      prev = no;
    }
  }
  for (int g = 0; g < 32; g++) {
    const int j0 = 2 * g, j1 = 2 * g + 1;
    auto entry = [&](int i) { return &out[((size_t)i * 32 + g) * 4]; };
    for (int i = 0; i < 3; i++) {
      float *e = entry(i);
      e[0] = Wl[0][j0 * kNetIn + 2 * i]; e[1] = Wl[0][j1 * kNetIn + 2 * i];
      e[2] = Wl[0][j0 * kNetIn + 2 * i + 1]; e[3] = Wl[0][j1 * kNetIn + 2 * i + 1];
    }
    for (int l = 0; l < NHID; l++) {
      float *e = entry(3 + l / 2) + 2 * (l & 1);
      e[0] = Bl[l][j0] * kTanhScale; e[1] = Bl[l][j1] * kTanhScale;
    }
    const int row = g >> 4, b3 = (g >> 3) & 1;
    const int qa = b3, qb = 1 - b3, pa = 2 + b3, pb = 3 - b3;
    const float *W3 = Wl[NHID];
    float *q = entry(3 + NB), *pp = entry(4 + NB), *c = entry(5 + NB);
    q[0] = W3[qa * H + j0]; q[1] = W3[qb * H + j0]; q[2] = W3[qa * H + j1]; q[3] = W3[qb * H + j1];
    pp[0] = W3[pa * H + j0]; pp[1] = W3[pb * H + j0]; pp[2] = W3[pa * H + j1]; pp[3] = W3[pb * H + j1];
    c[0] = Bl[NHID][2 * row + b3];
  }
  float *lds = out.data() + (size_t)NE * 32 * 4;
  for (int l = 1; l < NHID; l++)
    for (int k = 0; k < H; k++)
      for (int g = 0; g < 32; g++) {
        float *e = lds + (((size_t)(l - 1) * H + k) * 32 + g) * 2;
        e[0] = Wl[l][(2 * g) * H + k];
        e[1] = Wl[l][(2 * g + 1) * H + k];
      }
  return out;
}

// Image of the 4x4x1-MFMA form (rollout_m44.hip): float4 q of lane l at float4 index q * 64 + l.  Lane l holds ITS neuron's
// rows (B operands) of layer 0 and of the hidden layers, its hidden biases times kTanhScale, and -- for the output layer,
// which reduces over the lanes -- the weights of outputs {0,1} and {2,3} for the four activations 4 (l >> 2) + s of its block.
std::vector<float> pack_m44_weights(const std::vector<float> &theta, int NHID)
{
  const int H = 64, qb = 2, qh = 2 + (NHID + 3) / 4, qo = qh + (NHID - 1) * 16, qt = qo + 5;
  std::vector<float> out((size_t)qt * 64 * 4, 0.0f);
  std::vector<const float *> Wl(NHID + 1), Bl(NHID + 1);
  {
    const float *p = theta.data();
    int prev = kNetIn;
    for (int l = 0; l <= NHID; l++) {
      const int no = (l < NHID) ? H : kNetOut;
      Wl[l] = p;
      Bl[l] = p + (size_t)no * prev;
      p += (size_t)no * prev + no;
      prev = no;
    }
  }
  for (int l = 0; l < 64; l++) {
    auto at = [&](int e) -> float & { return out[((size_t)(e >> 2) * 64 + l) * 4 + (e & 3)]; };
    for (int c = 0; c < kNetIn; c++) at(c) = Wl[0][l * kNetIn + c];
    for (int j = 0; j < NHID; j++) at(4 * qb + j) = Bl[j][l] * kTanhScale;
    for (int j = 1; j < NHID; j++)
      for (int k = 0; k < H; k++) at(4 * (qh + 16 * (j - 1)) + k) = Wl[j][l * H + k];
    const int b = l >> 2;
    const float *W3 = Wl[NHID];
    for (int s = 0; s < 4; s++) {
      at(4 * qo + 2 * s) = W3[0 * H + 4 * b + s];
      at(4 * qo + 2 * s + 1) = W3[1 * H + 4 * b + s];
      at(4 * (qo + 2) + 2 * s) = W3[2 * H + 4 * b + s];
      at(4 * (qo + 2) + 2 * s + 1) = W3[3 * H + 4 * b + s];
    }
    at(4 * (qo + 4)) = Bl[NHID][l >> 4];
  }
  return out;
}

// Image of the LDS form on the 4x4x1 MFMA (rollout_lds44.hip), any layer list with hidden widths <= 64: float4 q of lane l at
// float4 index q * 64 + l.  First kLds44BiasQuads quads: float e of lane l = bias of layer e (hidden layers: b[l] x kTanhScale;
// output layer: b_out[l >> 4]).  Then per layer ceil(nin / 4) quads, quad q' = (W[l][4 q'] .. W[l][4 q' + 3]) -- lane l is neuron
// l, the B operand of k steps 4 q' .. 4 q' + 3 -- with the output layer's row c at lane 16 c.  Then kLds44Ahead quads the
// kernel's read-ahead may touch.  Every entry without a weight (k >= nin, l >= nout, the other lanes of the output layer) is 0.
std::vector<float> pack_lds44_weights(const std::vector<float> &theta, const NetDesc &net)
{
  std::vector<float> out((size_t)lds44_pack_floats(net), 0.0f);
  const int n_w = net.n_layers - 1;
  const float *p = theta.data();
  int q0 = kLds44BiasQuads;
  for (int j = 0; j < n_w; j++) {
    const int nin = net.layers[j], nout = net.layers[j + 1];
    const float *W = p, *B = p + (size_t)nout * nin;
    const bool last = j == n_w - 1;
    for (int l = 0; l < 64; l++) {
      auto at = [&](int e) -> float & { return out[((size_t)(e >> 2) * 64 + l) * 4 + (e & 3)]; };
      const int n = last ? ((l & 15) == 0 ? (l >> 4) : -1) : (l < nout ? l : -1);  // the neuron whose row lane l holds
      at(j) = last ? B[l >> 4] : (n >= 0 ? B[n] * kTanhScale : 0.0f);
      if (n >= 0)
        for (int k = 0; k < nin; k++) at(4 * q0 + k) = W[(size_t)n * nin + k];
    }
    q0 += (nin + 3) / 4;
    p += (size_t)nout * nin + nout;
  }
  return out;
}

// Image of the two-half LDS form (rollout_lds128.hip), any layer list with hidden widths <= 128: float4 q of lane l at float4
// index q * 64 + l.  First kLds128BiasQuads quads: float e = 2 j + h of lane l = bias of neuron 64 h + l of weight layer j (hidden
// layers: b x kTanhScale, 0 where the neuron does not exist; output layer, e = 2 j: b_out[l >> 4]).  Then per weight layer
// ceil(nin / 4) x H quads, H = ceil(nout / 64) halves (1 for the output layer), interleaved: quad q' H + h of the layer is
// (W[64 h + l][4 q'] .. W[64 h + l][4 q' + 3]) -- lane l is neuron 64 h + l, the B operand of k steps 4 q' .. 4 q' + 3 of
// accumulator h -- with the output layer's row c at lane 16 c.  Then kLds44Ahead quads the kernel's read-ahead may touch.  Every
// entry without a weight (k >= nin, 64 h + l >= nout, the other lanes of the output layer) is 0.
std::vector<float> pack_lds128_weights(const std::vector<float> &theta, const NetDesc &net)
{
  std::vector<float> out((size_t)lds128_pack_floats(net), 0.0f);
  const int n_w = net.n_layers - 1;
  const float *p = theta.data();
  int q0 = kLds128BiasQuads;
  for (int j = 0; j < n_w; j++) {
    const int nin = net.layers[j], nout = net.layers[j + 1];
    const float *W = p, *B = p + (size_t)nout * nin;
    const bool last = j == n_w - 1;
    const int H = (!last && nout > 64) ? 2 : 1;
    for (int h = 0; h < H; h++)
      for (int l = 0; l < 64; l++) {
        auto at = [&](int q, int c) -> float & { return out[((size_t)q * 64 + l) * 4 + c]; };
        const int n = last ? ((l & 15) == 0 ? (l >> 4) : -1) : (64 * h + l < nout ? 64 * h + l : -1);  // the neuron whose row lane l holds
        const int e = 2 * j + h;
        at(e >> 2, e & 3) = last ? B[l >> 4] : (n >= 0 ? B[n] * kTanhScale : 0.0f);
        if (n >= 0)
          for (int k = 0; k < nin; k++) at(q0 + (k >> 2) * H + h, k & 3) = W[(size_t)n * nin + k];
      }
    q0 += ((nin + 3) / 4) * H;
    p += (size_t)nout * nin + nout;
  }
  return out;
}

// Image of the 16x16x4 LDS form (rollout_lds16.hip), any layer list with hidden widths <= 128, in float4 ("quads"); lane l =
// (row = l & 15, kk = l >> 4), the neuron of row `row` of tile m is n = 16 m + 4 (row & 3) + (row >> 2) (the output layer: row & 3).
//   biases   weight layer j at quad boff[j]: hidden layers 4 MT_j quads, quad 4 m + g = kTanhScale x (b[16 m + g], b[16 m + 4 + g],
//            b[16 m + 8 + g], b[16 m + 12 + g]); the output layer ONE quad b_out[0..3]
//   layer 0  at quad off[0]: MT_0 half blocks of 32 quads, float2 l of half block m = (W[n][kk], W[n][4 + kk]), 0 for k >= 6
//   layer j  at quad off[j]: blocks of 64 quads, quad l of block (m, mi) = (W[n][16 mi + kk], W[n][16 mi + 4 + kk], W[n][16 mi + 8 + kk],
//            W[n][16 mi + 12 + kk]) -- k-steps 4 mi .. 4 mi + 3 of tile m -- in the order of their use: block index 2 (P MT_in + mi) + h
//            for tile m = 2 P + h of a pair, and (MT_j - 1) MT_in + mi for an odd last tile (MT_in = MT_(j-1) input tiles)
//   then kLds16Ahead = 2 blocks the kernel's read-ahead may touch.
// Every entry without a weight (a neuron or an input that does not exist) is 0.
// pack_mfma16_image: the image of descriptor d (lds16_net_of / glb16_net_of: up to 8 / 16 tiles per layer) in `floats` floats
static std::vector<float> pack_mfma16_image(const std::vector<float> &theta, const NetDesc &net, const Lds16Net &d, size_t floats)
{
  std::vector<float> out(floats, 0.0f);
  const float *p = theta.data();
  for (int j = 0; j < d.n_w; j++) {
    const int nin = net.layers[j], nout = net.layers[j + 1];
    const float *W = p, *B = p + (size_t)nout * nin;
    const bool last = j == d.n_w - 1;
    float *bq = out.data() + 4 * (size_t)d.boff[j];
    if (last) {
      for (int r = 0; r < 4; r++) bq[r] = B[r];
    } else {
      for (int m = 0; m < d.mt[j]; m++)
        for (int g = 0; g < 4; g++)
          for (int r = 0; r < 4; r++) {
            const int n = 16 * m + 4 * r + g;
            if (n < nout) bq[(4 * m + g) * 4 + r] = B[n] * kTanhScale;
          }
    }
    float *wq = out.data() + 4 * (size_t)d.off[j];
    const int mt_in = j == 0 ? 1 : d.mt[j - 1];
    for (int m = 0; m < d.mt[j]; m++)
      for (int l = 0; l < 64; l++) {
        const int row = l & 15, kk = l >> 4;
        const int n = last ? (row & 3) : 16 * m + 4 * (row & 3) + (row >> 2);
        if (n >= nout) continue;
        if (j == 0) {
          for (int c = 0; c < 2; c++)
            if (4 * c + kk < nin) wq[((size_t)m * 64 + l) * 2 + c] = W[(size_t)n * nin + 4 * c + kk];
          continue;
        }
        for (int mi = 0; mi < mt_in; mi++) {
          const bool odd_tail = (d.mt[j] & 1) && m == d.mt[j] - 1;
          const size_t block = odd_tail ? (size_t)m * mt_in + mi : 2 * ((size_t)(m >> 1) * mt_in + mi) + (m & 1);
          for (int c = 0; c < 4; c++) {
            const int kap = 16 * mi + 4 * c + kk;
            if (kap < nin) wq[(block * 64 + l) * 4 + c] = W[(size_t)n * nin + kap];
          }
        }
      }
    p += (size_t)nout * nin + nout;
  }
  return out;
}
std::vector<float> pack_lds16_weights(const std::vector<float> &theta, const NetDesc &net)
{
  const size_t floats = (size_t)lds16_pack_floats(net);
  return floats ? pack_mfma16_image(theta, net, lds16_net_of(net), floats) : std::vector<float>();
}
// Image of rollout_glb16.hip, any layer list with hidden widths <= 256: the layout above with up to 16 tiles per layer and
// kGlb16Ahead blocks of zeros behind the stream
std::vector<float> pack_glb16_weights(const std::vector<float> &theta, const NetDesc &net)
{
  const size_t floats = (size_t)glb16_pack_floats(net);
  return floats ? pack_mfma16_image(theta, net, glb16_net_of(net), floats) : std::vector<float>();
}
// Image of rollout_glb44.hip, any layer list with hidden widths <= 256, in 1 KB quads: float4 q of lane l at float4 index q * 64 + l.
// First kGlb44BiasQuads quads: float h of quad j of lane l = bias of neuron 64 h + l of weight layer j (hidden layers: b x
// kTanhScale, 0 where the neuron does not exist; output layer, float 0: b_out[l >> 4]).  Then per weight layer ceil(nin / 4) x H
// quads, H = ceil(nout / 64) halves (1 for the output layer), interleaved in the order of their use: quad q' H + h of the layer is
// (W[64 h + l][4 q'] .. W[64 h + l][4 q' + 3]), the output layer's row c at lane 16 c.  Then kGlb44Ahead quads of zeros.  Every entry
// without a weight is 0.  Behind the bias quads the weights are pack_lds128_weights' float for float on a list that form serves.
std::vector<float> pack_glb44_weights(const std::vector<float> &theta, const NetDesc &net)
{
  std::vector<float> out((size_t)glb44_pack_floats(net), 0.0f);
  if (out.empty()) return out;
  const int n_w = net.n_layers - 1;
  const float *p = theta.data();
  int q0 = kGlb44BiasQuads;
  for (int j = 0; j < n_w; j++) {
    const int nin = net.layers[j], nout = net.layers[j + 1];
    const float *W = p, *B = p + (size_t)nout * nin;
    const bool last = j == n_w - 1;
    const int H = last ? 1 : (nout + 63) / 64;
    for (int h = 0; h < H; h++)
      for (int l = 0; l < 64; l++) {
        auto at = [&](int q, int c) -> float & { return out[((size_t)q * 64 + l) * 4 + c]; };
        const int n = last ? ((l & 15) == 0 ? (l >> 4) : -1) : (64 * h + l < nout ? 64 * h + l : -1);  // the neuron whose row lane l holds
        at(j, h) = last ? B[l >> 4] : (n >= 0 ? B[n] * kTanhScale : 0.0f);
        if (n >= 0)
          for (int k = 0; k < nin; k++) at(q0 + (k >> 2) * H + h, k & 3) = W[(size_t)n * nin + k];
      }
    q0 += ((nin + 3) / 4) * H;
    p += (size_t)nout * nin + nout;
  }
  return out;
}

int seed_device(mppi_handle *h, uint64_t seed, uint64_t offset)
{
  // base state: L'Ecuyer's default 12345 x 6, scrambled by the seed (DESIGN.md noise spec)
  uint32_t base[6] = {12345u, 12345u, 12345u, 12345u, 12345u, 12345u};
  if (seed != 0) {
    const uint32_t x1 = ((uint32_t)seed) ^ 0x55555555u;
    const uint32_t x2 = (uint32_t)((seed >> 32) ^ 0xAAAAAAAAu);
    base[0] = (uint32_t)((uint64_t)x1 * base[0] % M1);
    base[1] = (uint32_t)((uint64_t)x2 * base[1] % M1);
    base[2] = (uint32_t)((uint64_t)x1 * base[2] % M1);
    base[3] = (uint32_t)((uint64_t)x2 * base[3] % M2);
    base[4] = (uint32_t)((uint64_t)x1 * base[4] % M2);
    base[5] = (uint32_t)((uint64_t)x2 * base[5] % M2);
  }
  int sub_bits = 0;
  while ((1LL << sub_bits) < (long long)h->K) sub_bits++;
  HIPCHK(h, launch_noise_init(h->d_rng[0], h->K, base, h->d_sub, sub_bits, h->d_one, offset, h->stream));
  h->rng_cur = 0;
  h->cfg.seed = seed;
  return MPPI_OK;
}

int upload_rng_tables(mppi_handle *h)
{
  std::vector<uint32_t> sub(32 * 18), one(64 * 18), jump((size_t)h->noise_C * 18);
  Mat3 a1 = base_A1(), a2 = base_A2();
  for (int b = 0; b < 64; b++) {  // A^(2^b)
    memcpy(&one[(size_t)b * 18], a1.a, 36);
    memcpy(&one[(size_t)b * 18 + 9], a2.a, 36);
    a1 = mat_mul(a1, a1, M1);
    a2 = mat_mul(a2, a2, M2);
  }
  for (int b = 64; b < 76; b++) {
    a1 = mat_mul(a1, a1, M1);
    a2 = mat_mul(a2, a2, M2);
  }
  for (int b = 0; b < 32; b++) {  // A^(2^76 * 2^b)
    memcpy(&sub[(size_t)b * 18], a1.a, 36);
    memcpy(&sub[(size_t)b * 18 + 9], a2.a, 36);
    a1 = mat_mul(a1, a1, M1);
    a2 = mat_mul(a2, a2, M2);
  }
  const Mat3 j1 = mat_pow(base_A1(), 2ULL * (uint64_t)h->noise_L, M1);
  const Mat3 j2 = mat_pow(base_A2(), 2ULL * (uint64_t)h->noise_L, M2);
  Mat3 c1 = mat_identity(), c2 = mat_identity();
  for (int c = 0; c < h->noise_C; c++) {  // A^(2 L c)
    memcpy(&jump[(size_t)c * 18], c1.a, 36);
    memcpy(&jump[(size_t)c * 18 + 9], c2.a, 36);
    c1 = mat_mul(j1, c1, M1);
    c2 = mat_mul(j2, c2, M2);
  }
  HIPCHK(h, hipMemcpy(h->d_sub, sub.data(), sub.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_one, one.data(), one.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_jump, jump.data(), jump.size() * 4, hipMemcpyHostToDevice));
  return MPPI_OK;
}

// Image of rollout_trace.hip: theta's own layout [W1|b1|W2|b2|...] with every W transposed to k-major [nin][nout], so that
// the lanes of a wavefront (one neuron each) read contiguous floats for one k; biases as they are.
std::vector<float> pack_trace_weights(const std::vector<float> &theta, const mppi::NetDesc &net)
{
  std::vector<float> img(theta.size());
  size_t off = 0;
  for (int l = 0; l + 1 < net.n_layers; l++) {
    const size_t nin = net.layers[l], nout = net.layers[l + 1];
    for (size_t j = 0; j < nout; j++)
      for (size_t k = 0; k < nin; k++) img[off + k * nout + j] = theta[off + j * nin + k];
    for (size_t j = 0; j < nout; j++) img[off + nin * nout + j] = theta[off + nin * nout + j];
    off += nin * nout + nout;
  }
  return img;
}


// The weight images, one row per Image: which handles have one, its size in floats, how it is packed from h->theta.
namespace {
using H = const mppi_handle *;
size_t num_params(H h) { return (size_t)h->net.num_params; }
// theta with the hidden-layer biases pre-scaled for tanh_bias
std::vector<float> pack_scaled_theta(H h)
{
  std::vector<float> ts(h->theta);
  size_t off = 0;
  for (int l = 0; l + 1 < h->net.n_layers; l++) {
    const size_t nin = h->net.layers[l], nout = h->net.layers[l + 1];
    if (l + 2 < h->net.n_layers)
      for (size_t j = 0; j < nout; j++) ts[off + nin * nout + j] = ts[off + nin * nout + j] * kTanhScale;
    off += nin * nout + nout;
  }
  return ts;
}
constexpr ImageDesc kImages[] = {
    // image, which handles have it, floats, packed image, built on request, size check
    {Image::Theta, [](H) { return true; }, num_params, [](H h) { return h->theta; }, false, nullptr},
    {Image::ThetaS, [](H h) { return !h->basis; }, num_params, pack_scaled_theta, false, nullptr},
    {Image::Mfma, [](H h) { return h->mfma_ok; }, [](H h) { return (size_t)64 * mfma_pack_floats_per_lane(h->hidden, h->n_hidden); },
     [](H h) { return pack_mfma_weights(h->theta, h->hidden, h->n_hidden); }, false, nullptr},
    {Image::Row, [](H h) { return h->mfma_ok && row_variant_supported(h->hidden, h->n_hidden); }, [](H) { return (size_t)row_pack_floats(); },
     [](H h) { return pack_row_weights(h->theta); }, false, nullptr},
    {Image::BfRow, [](H h) { return h->basis; }, [](H) { return (size_t)bf_row_pack_floats(); }, [](H h) { return pack_bf_row_weights(h->theta); }, false, nullptr},
    {Image::Row64, [](H h) { return h->mfma_ok && row64_variant_supported(h->hidden, h->n_hidden); }, [](H h) { return (size_t)row64_pack_floats(h->n_hidden); },
     [](H h) { return pack_row64_weights(h->theta, h->n_hidden); }, false, nullptr},
    {Image::M44, [](H h) { return h->mfma_ok && m44_variant_supported(h->hidden, h->n_hidden); }, [](H h) { return (size_t)m44_pack_floats(h->n_hidden); },
     [](H h) { return pack_m44_weights(h->theta, h->n_hidden); }, false, "m44 image size"},
    {Image::Lds44, [](H h) { return !h->basis && lds44_supported(h->net); }, [](H h) { return (size_t)lds44_pack_floats(h->net); },
     [](H h) { return pack_lds44_weights(h->theta, h->net); }, false, nullptr},
    {Image::Lds128, [](H h) { return !h->basis && lds128_supported(h->net); }, [](H h) { return (size_t)lds128_pack_floats(h->net); },
     [](H h) { return pack_lds128_weights(h->theta, h->net); }, false, "lds128 image size"},
    {Image::Lds16, [](H h) { return !h->basis && lds16_supported(h->net); }, [](H h) { return (size_t)lds16_pack_floats(h->net); },
     [](H h) { return pack_lds16_weights(h->theta, h->net); }, false, "lds16 image size"},
    {Image::Glb16, [](H h) { return !h->basis && glb16_supported(h->net); }, [](H h) { return (size_t)glb16_pack_floats(h->net); },
     [](H h) { return pack_glb16_weights(h->theta, h->net); }, true, "glb16 image size"},
    {Image::Glb44, [](H h) { return !h->basis && glb44_supported(h->net); }, [](H h) { return (size_t)glb44_pack_floats(h->net); },
     [](H h) { return pack_glb44_weights(h->theta, h->net); }, true, "glb44 image size"},
    {Image::Row32, [](H h) { return !h->basis && row32_supported(h->net, true); }, [](H h) { return (size_t)row32_pack_floats(h->net); },
     [](H h) { return pack_row32_weights(h->theta, h->net); }, true, "row32 image size"},
    {Image::Trace, [](H h) { return !h->basis; }, num_params, [](H h) { return pack_trace_weights(h->theta, h->net); }, false, nullptr},
};
static_assert(rows_in_order(kImages, &ImageDesc::id), "row i of kImages describes image i");
}  // namespace
const ImageDesc &image_desc(Image id) { return kImages[(int)id]; }

int upload_image(mppi_handle *h, Image id)
{
  const ImageDesc &im = image_desc(id);
  DeviceImage &di = h->img[(int)id];
  const std::vector<float> pk = im.pack(h);
  if (im.on_request) {  // of a handle that asked for the form by name: allocated at the first call, rebuilt from h->theta at every call
    if (pk.empty() || h->theta.size() != (size_t)h->net.num_params) return fail(h, MPPI_ERR_INVALID, im.size_check);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!di.d) {
      di.bytes = pk.size() * sizeof(float);
      HIPCHK(h, hipMalloc(&di.d, di.bytes));
    }
  }
  if (im.size_check && pk.size() * sizeof(float) != di.bytes) return fail(h, MPPI_ERR_INVALID, im.size_check);
  if (im.on_request) HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(di.d, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
  return MPPI_OK;
}

int upload_images(mppi_handle *h)
{
  for (const ImageDesc &im : kImages) {
    const bool wanted = im.on_request && form_desc(h->forced).image == im.id;  // asked for before the parameters were set
    if (h->img[(int)im.id].d || wanted)
      if (int rc = upload_image(h, im.id)) return rc;
  }
  return MPPI_OK;
}

}  // namespace mppi_abi
