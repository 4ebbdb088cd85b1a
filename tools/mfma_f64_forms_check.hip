// v_mfma_f64_16x16x4 against four v_mfma_f64_4x4x4_4b on gfx950: does one output element get the same BITS from both forms?
// Both add the same four products of a k-step to the same accumulator, k-steps in the same order; whether the hardware rounds them
// alike is what this program finds out.  One workgroup of one wave runs a chain of 13 k-steps (the C2 strip product, KW = 13) into
// one 16 x 16 accumulator tile, once with the large instruction and once with the small one on each of the tile's four components,
// operands in the layouts of a strip product (csrc/mom_strip.hpp):
//   B: lane l holds X[4 ks + (l >> 4)][l & 15] -- the same register for both forms;
//   D: lane l, component r holds row 4 r + (l >> 4), column l & 15 -- the same registers for both forms;
//   A: large form M[4 ks + (l >> 4)][l & 15]; small form, component r, M[4 ks + (l >> 4)][4 r + (l & 3)] -- the same 4 x 4 block in
//      all four lane groups (the broadcast read of csrc/mom_q4.hpp q4_mul_c).
// Three magnitude mixes, kTrials seeded draws each: normal; exponents spread over +-300 with both signs (terms of one sum up to 2^1200
// apart, cancellation); exact zeros and subnormals among normal values.  Prints the number of differing
// elements per mix (memcmp per element) and exits 1 if there is any.
//   hipcc -O3 --offload-arch=gfx950 tools/mfma_f64_forms_check.hip -o mfma_f64_forms_check
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kSteps = 13, kK = 4 * kSteps, kTrials = 64;

// M: kK x 16 (k-major: M[k * 16 + row]), X: kK x 16 (X[k * 16 + col]), C: 16 x 16 (C[row * 16 + col]); D16, D4: 16 x 16 likewise
__global__ void __launch_bounds__(64) k_forms(const double *M, const double *X, const double *C, double *D16, double *D4) {
  const int l = threadIdx.x, lr = l & 15, lq = l >> 4;
  d4 big, small;
  for (int r = 0; r < 4; ++r) big[r] = small[r] = C[(4 * r + lq) * 16 + lr];
#pragma unroll
  for (int ks = 0; ks < kSteps; ++ks) {
    const double b = X[(4 * ks + lq) * 16 + lr];
    const double a = M[(4 * ks + lq) * 16 + lr];
    double a4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a4[r] = M[(4 * ks + lq) * 16 + 4 * r + (l & 3)];
    big = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, big, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) small[r] = __builtin_amdgcn_mfma_f64_4x4x4f64(a4[r], b, small[r], 0, 0, 0);
  }
  for (int r = 0; r < 4; ++r) {
    D16[(4 * r + lq) * 16 + lr] = big[r];
    D4[(4 * r + lq) * 16 + lr] = small[r];
  }
}

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double uni() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
static double draw(int mix) {
  const double s = (rng() & 1) ? -1.0 : 1.0, m = 0.5 + uni();
  if (mix == 0) return s * m;
  if (mix == 1) return s * std::ldexp(m, (int)(rng() % 601) - 300);
  switch (rng() % 4) {
    case 0: return (rng() & 1) ? 0.0 : -0.0;
    case 1: return s * std::ldexp(m, -1040 - (int)(rng() % 34));  // subnormal
    case 2: return s * std::ldexp(m, -520 + (int)(rng() % 8) - 4);  // products of two land around the subnormal range
    default: return s * m;
  }
}

#define CHECK(x)                                                                      \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      printf("%s: %s\n", #x, hipGetErrorString(e_));                                  \
      return 2;                                                                       \
    }                                                                                 \
  } while (0)

int main() {
  double *dM, *dX, *dC, *dA, *dB;
  CHECK(hipMalloc(&dM, kK * 16 * 8));
  CHECK(hipMalloc(&dX, kK * 16 * 8));
  CHECK(hipMalloc(&dC, 256 * 8));
  CHECK(hipMalloc(&dA, 256 * 8));
  CHECK(hipMalloc(&dB, 256 * 8));
  std::vector<double> M(kK * 16), X(kK * 16), C(256), A(256), B(256);
  static const char *names[3] = {"normal", "exponents +-300, both signs", "zeros and subnormals"};
  long total = 0;
  for (int mix = 0; mix < 3; ++mix) {
    long diff = 0, nonfinite = 0, subn = 0;
    for (int t = 0; t < kTrials; ++t) {
      rng_state = 0x5EEDull + 1000003ull * (uint64_t)(mix * kTrials + t);
      for (auto &v : M) v = draw(mix);
      for (auto &v : X) v = draw(mix);
      for (auto &v : C) v = (t & 1) ? draw(mix) : 0.0;  // every other draw starts from a zero accumulator, as strip_zero does
      CHECK(hipMemcpy(dM, M.data(), M.size() * 8, hipMemcpyHostToDevice));
      CHECK(hipMemcpy(dX, X.data(), X.size() * 8, hipMemcpyHostToDevice));
      CHECK(hipMemcpy(dC, C.data(), C.size() * 8, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_forms, dim3(1), dim3(64), 0, 0, dM, dX, dC, dA, dB);
      CHECK(hipGetLastError());
      CHECK(hipMemcpy(A.data(), dA, 256 * 8, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(B.data(), dB, 256 * 8, hipMemcpyDeviceToHost));
      for (int e = 0; e < 256; ++e) {
        if (std::memcmp(&A[e], &B[e], 8) != 0) {
          if (diff < 8) printf("  mix %d draw %d element (%d, %d): 16x16x4 %a  4x4x4 %a\n", mix, t, e / 16, e % 16, A[e], B[e]);
          ++diff;
        }
        if (!std::isfinite(A[e])) ++nonfinite;
        else if (A[e] != 0.0 && std::fabs(A[e]) < 2.2250738585072014e-308) ++subn;
      }
    }
    printf("%-28s: %d draws x 256 elements, %ld differ (%ld non-finite, %ld subnormal results)\n", names[mix], kTrials, diff, nonfinite,
           subn);
    total += diff;
  }
  printf("differing elements: %ld\n", total);
  return total ? 1 : 0;
}
