// K7: score ranking. The reference sorts the gathered CTR list ascending with
// Collections.sort on boxed Floats and in doing so loses which candidate each
// score belongs to (reference DCNClient.java:195). Here one workgroup sorts up
// to 8192 (score, candidate) pairs in LDS with a bitonic network and returns
// both the sorted scores and the permutation; top-k is a prefix of it.
#include "common.h"
#include "launchers.h"

namespace dtfs {
namespace kern {

constexpr int kSortMax = 8192;

// Total order on scores as an unsigned key: the IEEE bits made monotonic
// (-inf lowest, +inf highest, -0.0 == +0.0 so zeros tie like in a comparison
// sort), inverted for descending; NaN ranks after every number in both modes
// and padding after NaN.
constexpr uint32_t kSortKeyNaN = 0xfffffffeu, kSortKeyPad = 0xffffffffu;

__device__ __forceinline__ uint32_t sort_key(float v, bool descending) {
  if (v != v) return kSortKeyNaN;
  uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // [0x007fffff (-inf), 0xff800000 (+inf)]
  return descending ? ~u : u;
}

__global__ void __launch_bounds__(1024) bitonic_sort_kernel(const float* __restrict__ in, int n, int descending,
                                                            float* __restrict__ out, int64_t* __restrict__ perm,
                                                            int k_out) {
  __shared__ uint32_t key[kSortMax];
  __shared__ int idx[kSortMax];
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  // Always sort ascending on the transformed key, so ties break by candidate
  // index in both modes; NaN and padding rank last.
  for (int i = threadIdx.x; i < p2; i += blockDim.x) {
    key[i] = i < n ? sort_key(in[i], descending != 0) : kSortKeyPad;
    idx[i] = i < n ? i : 0x7fffffff;
  }
  __syncthreads();
  for (int size = 2; size <= p2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < p2 / 2; i += blockDim.x) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint32_t a = key[lo], b = key[hi];
        const int ia = idx[lo], ib = idx[hi];
        // total order: by key, ties by candidate index (stable)
        const bool gt = (a > b) || (a == b && ia > ib);
        if (gt == up) {
          key[lo] = b;
          key[hi] = a;
          idx[lo] = ib;
          idx[hi] = ia;
        }
      }
      __syncthreads();
    }
  }
  // the scores themselves, bit for bit (the key folds -0.0 and every NaN)
  for (int i = threadIdx.x; i < k_out; i += blockDim.x) {
    const int j = idx[i];
    out[i] = in[j];
    if (perm) perm[i] = j;
  }
}

}  // namespace kern

using namespace kern;

int sort_max_elems() { return kSortMax; }

hipError_t launch_sort_scores(const float* in, int n, bool descending, float* out, int64_t* perm, int k_out,
                              hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > kSortMax || k_out > n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bitonic_sort_kernel, dim3(1), dim3(1024), 0, st, in, n, descending ? 1 : 0, out, perm, k_out);
  return hipGetLastError();
}

}  // namespace dtfs
