// bf_row_ub.hip -- the dynamics step of the basis-function model alone on a SIMD, one wavefront per SIMD, in its two layouts:
//   lane form: one lane per rollout (rollout_bf.hip: basis_shared_fast, basis_funcs_from, basis_dynamics_dev) -- a wavefront
//              steps 64 rollouts;
//   row form:  a rollout's sixteen (output, y-thread) cells on one DPP row (rollout_bf_row.hip: bf_row_deriv, the four row
//              broadcasts of the new state) -- a wavefront steps 4 rollouts;
//   row form + book: with the per-step bookkeeping of the product's dynamics wave (the state record and the sequence word to LDS,
//              the control wave's count and the next controls from LDS, the scalar end-of-step test that never waits here).
// Cycles per step of the recurrence (s_memtime over `iters` steps), and the states after the last step compared bit for bit:
// the rollouts of the row form start from the states of the lane form's first rollouts and take the same controls.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/ub/bf_row_ub.hip -o bf_row_ub -Lautorally_amd -lmppi_hip -Wl,-rpath,$PWD/autorally_amd
#include "../../autorally_amd/csrc/bf_row_device.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace mppi;

namespace mppi_abi { std::vector<float> pack_bf_row_weights(const std::vector<float> &W); }

__device__ __forceinline__ void start_state(int k, float *s)  // s3..s6 of rollout k
{
  s[0] = 0.002f * (float)(k % 64) - 0.05f; s[1] = 4.0f + 0.03f * (float)(k % 50); s[2] = 0.1f - 0.004f * (float)(k % 40); s[3] = 0.01f * (float)(k % 30);
}
__device__ __forceinline__ f32x2 control(int t) { return f32x2{0.05f - 0.01f * (float)(t & 7), 0.3f + 0.01f * (float)(t & 3)}; }

__global__ __launch_bounds__(256) void k_lane(const float *W, float *out, unsigned long long *cyc, int iters, float dt)
{
  __shared__ __attribute__((aligned(16))) float W_s[4 * kNumBfs];  // transposed: [25][4]
  for (int i = threadIdx.x; i < 4 * kNumBfs; i += 256) W_s[(i % kNumBfs) * 4 + i / kNumBfs] = W[i];
  __syncthreads();
  BfWeights Wr;
  Wr.load(W_s);
  const int k = blockIdx.x * 256 + threadIdx.x;
  float s[kStateDim] = {0, 0, 0, 0, 0, 0, 0};
  start_state(k, s + 3);
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  for (int t = 0; t < iters; t++) {
    const f32x2 u = control(t);
    float phi[kNumBfs], d[4];
    BasisShared c;
    basis_shared_fast(s, u.x, c);
    basis_funcs_from(s, u.y, c, phi);
    basis_dynamics_dev(Wr, phi, d);
#pragma unroll
    for (int i = 0; i < 4; i++) s[3 + i] = fmaf(d[i], dt, s[3 + i]);
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = c1 - c0;
#pragma unroll
  for (int i = 0; i < 4; i++) out[k * 4 + i] = s[3 + i];
}

struct BookLds {
  float rec[kGRing][16][4];
  float ctl[kGRing][16][4];
  int seq[4][64], pub[64];
  float dump[4][64];
};
template <bool BOOK>
__global__ __launch_bounds__(256) void k_row(const float *pack, float *out, unsigned long long *cyc, int iters, float dt)
{
  __shared__ __attribute__((aligned(16))) BookLds L;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane >> 4, p = lane & 15, j = p >> 2, y = p & 3;
  const int jr = 4 * w + r;
  const int k = blockIdx.x * 16 + jr;
  BfRowLane Ln;
  bf_row_load(pack, p, Ln);
  if (w == 0) L.pub[lane] = 1 << 30;
  for (int i = threadIdx.x; i < kGRing * 16 * 4; i += 256) (&L.ctl[0][0][0])[i] = 0.1f;
  __syncthreads();
  typedef const volatile int __attribute__((address_space(3))) *lds_int_p;
  typedef const volatile f32x2 __attribute__((address_space(3))) *lds_f2_p;
  const lds_int_p p_pub = (lds_int_p)&L.pub[0];
  const lds_f2_p p_u = (lds_f2_p)&L.ctl[0][jr][0];
  const uint32_t a_myseq = lds_addr(&L.seq[w][lane]);
  const uint32_t a_rec0 = (y == 0) ? lds_addr(&L.rec[0][jr][j]) : lds_addr(&L.dump[w][lane]);
  const uint32_t rec_stride = (y == 0) ? 256u : 0u;
  float s0[4];
  start_state(k, s0);
  float s3 = s0[0], s4 = s0[1], s5 = s0[2], s6 = s0[3];
  float sj = bf_sel4(j, s3, s4, s5, s6);
  int budget = 1 << 20;
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  for (int t = 0; t < iters; t++) {
    f32x2 u = control(t);
    int cp_v = 1 << 30;
    if (BOOK) {
      asm volatile("ds_write_b32 %0, %1" ::"v"(a_rec0 + (uint32_t)(t & (kGRing - 1)) * rec_stride), "v"(sj) : "memory");
      lds_publish(a_myseq, t + 1);
      cp_v = *p_pub;
      const f32x2 un = p_u[((t + 1) & (kGRing - 1)) * 32];  // read as the product reads it; the controls stay control(t)
      u.x += 0.0f * un.x;
    }
    const float d = bf_row_deriv(Ln, y, s3, s4, s5, s6, u.x, u.y);
    sj = fmaf(d, dt, sj);
    s3 = bf_row_bc<0>(sj); s4 = bf_row_bc<4>(sj); s5 = bf_row_bc<8>(sj); s6 = bf_row_bc<12>(sj);
    if (BOOK) {
      int cp = __builtin_amdgcn_readfirstlane(cp_v);
      while (cp < t + 2 && --budget > 0) cp = __builtin_amdgcn_readfirstlane(*p_pub);
    }
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) cyc[blockIdx.x * 4 + w] = c1 - c0;
  if (y == 0) out[k * 4 + j] = sj + (float)(budget & 0);
}

int main(int argc, char **argv)
{
  const int iters = argc > 1 ? atoi(argv[1]) : 100;
  std::vector<float> W(4 * kNumBfs);
  for (size_t i = 0; i < W.size(); i++) W[i] = 0.5f * (float)((int)((i * 2654435761u) >> 20 & 255) - 128) / 128.0f;
  const std::vector<float> pk = mppi_abi::pack_bf_row_weights(W);
  float *d_W, *d_pk, *d_o;
  unsigned long long *d_c;
  const int NB = 256;               // one workgroup of four wavefronts per CU: one wavefront per SIMD
  const int NK = NB * 256;          // rollouts of the lane form; the row form steps the first NB * 16 of them
  hipMalloc(&d_W, W.size() * 4); hipMemcpy(d_W, W.data(), W.size() * 4, hipMemcpyHostToDevice);
  hipMalloc(&d_pk, pk.size() * 4); hipMemcpy(d_pk, pk.data(), pk.size() * 4, hipMemcpyHostToDevice);
  hipMalloc(&d_o, (size_t)NK * 16); hipMalloc(&d_c, NB * 4 * 8);
  const float dt = 0.02f;
  std::vector<float> ref((size_t)NK * 4), got((size_t)NK * 4);
  auto run = [&](const char *name, auto kern, const float *wts, int rollouts, bool is_ref) {
    hipMemset(d_o, 0, (size_t)NK * 16);
    for (int rep = 0; rep < 3; rep++) hipLaunchKernelGGL(kern, dim3(NB), dim3(256), 0, 0, wts, d_o, d_c, iters, dt);
    if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); return; }
    std::vector<unsigned long long> c(NB * 4);
    hipMemcpy(c.data(), d_c, c.size() * 8, hipMemcpyDeviceToHost);
    double s = 0;
    for (auto v : c) s += (double)v;
    hipMemcpy(is_ref ? ref.data() : got.data(), d_o, (size_t)NK * 16, hipMemcpyDeviceToHost);
    int bad = 0;
    if (!is_ref) for (int i = 0; i < rollouts * 4; i++) bad += memcmp(&ref[i], &got[i], 4) != 0;
    const double per_step = s / c.size() / iters;
    printf("%-52s %7.0f cycles per step, %2d rollouts per wavefront: %6.1f cycles per rollout step", name, per_step, rollouts / (NB * 4),
           per_step / (rollouts / (NB * 4)));
    if (!is_ref) printf("   %s (%d of %d words differ from the lane form)", bad ? "MISMATCH" : "bit-identical", bad, rollouts * 4);
    printf("\n");
  };
  printf("basis-function dynamics step, %d steps, one wavefront per SIMD\n", iters);
  run("lane form (bf3's dynamics wave)", k_lane, d_W, NK, true);
  run("row form (bf_row's dynamics wave), recurrence alone", k_row<false>, d_pk, NB * 16, false);
  run("row form + the product's per-step bookkeeping", k_row<true>, d_pk, NB * 16, false);
  return 0;
}
