// Recordings of any length in front of and behind the network (snrse.longform): a long recording is cut into
// overlapping windows of W samples that run as ordinary rows of the batched enhancers, and their results are joined
// by a cross-fade over the V samples at the head of every window but the first.
//
//   snrse_window_gather   ragged recordings [R][stride] + a table of (row, start, length) -> windows [nwin][W]
//   snrse_window_merge    window results [nwin][W] + the starts table -> ragged recordings [R][stride_out]
//
// The merge is in gather form: one thread per OUTPUT sample n of recording r.  With k the last window of r whose
// start s_k <= n (a binary search of the recording's slice of the starts table, uniform over all but a few waves)
//   k > 0 and n < s_k + V:  out = fma(t[n - s_k], x_k[n - s_k], (1 - t[n - s_k]) * x_{k-1}[n - s_{k-1}])
//   otherwise:              out = x_k[n - s_k]
// so at most two windows touch a sample, no atomics are needed, a launch repeats bit for bit and a recording's bits
// do not depend on the recordings it shares the launch with.  A window flagged silent contributes 0 and its buffer
// is not read.  Both kernels are streaming copies -- one dword per lane, consecutive lanes on consecutive
// addresses -- with every table entry clamped on the device: an entry that points outside its buffer yields zeros,
// never a read or a write out of bounds.  This file is compiled without fp contraction (snrse/build.py), so the
// cross-fade is exactly the expression above: four roundings (the table, 1 - t, the product, the fma).
#include "common.h"

namespace {

constexpr int WT = 256;  // threads per block = samples per block

__global__ __launch_bounds__(WT) void window_gather_kernel(const float* __restrict__ src,
                                                           const int* __restrict__ lengths, int R,
                                                           long long stride, const int* __restrict__ table,
                                                           int nwin, int W, float* __restrict__ out) {
  const int i = blockIdx.x * WT + threadIdx.x;
  if (i >= W) return;
  for (int j = blockIdx.y; j < nwin; j += gridDim.y) {
    const int row = table[3 * j], len = table[3 * j + 2];
    const long long s = table[3 * j + 1];
    float v = 0.0f;
    if (row >= 0 && row < R && s >= 0 && i < len) {
      long long L = lengths[row];
      L = L > stride ? stride : L;
      if (s + i < L) v = src[(size_t)row * (size_t)stride + (size_t)(s + i)];
    }
    out[(size_t)j * (size_t)W + (size_t)i] = v;
  }
}

__global__ __launch_bounds__(WT) void window_merge_kernel(const float* __restrict__ win, int nwin, int W,
                                                          const int* __restrict__ starts,
                                                          const unsigned char* __restrict__ silent,
                                                          const int* __restrict__ first,
                                                          const int* __restrict__ lengths, int R,
                                                          const float* __restrict__ fade, int V,
                                                          float* __restrict__ out, long long stride_out) {
  const long long n = (long long)blockIdx.x * WT + threadIdx.x;
  if (n >= stride_out) return;
  for (int r = blockIdx.y; r < R; r += gridDim.y) {
    float* o = out + (size_t)r * (size_t)stride_out + (size_t)n;
    int f0 = first[r], f1 = first[r + 1];
    f0 = f0 < 0 ? 0 : f0;
    f1 = f1 > nwin ? nwin : f1;
    if (n >= lengths[r] || f0 >= f1) {
      *o = 0.0f;
      continue;
    }
    // the last window j in [f0, f1) with starts[j] <= n (f0 when none is: its offset check below then fails)
    int lo = f0, hi = f1 - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (starts[mid] <= n) lo = mid; else hi = mid - 1;
    }
    const long long i = n - starts[lo];
    float v = 0.0f;
    if (i >= 0 && i < W) {
      v = silent[lo] ? 0.0f : win[(size_t)lo * (size_t)W + (size_t)i];
      const long long ip = n - starts[lo > f0 ? lo - 1 : lo];
      if (lo > f0 && i < V && ip >= 0 && ip < W) {
        const float t = fade[i];
        const float p = silent[lo - 1] ? 0.0f : win[(size_t)(lo - 1) * (size_t)W + (size_t)ip];
        v = fmaf(t, v, (1.0f - t) * p);
      }
    }
    *o = v;
  }
}

}  // namespace

extern "C" int snrse_window_gather(const float* src, const int* lengths, int R, long long stride, const int* table,
                                   int nwin, int W, float* out, hipStream_t stream) {
  if (!src || !lengths || !table || !out || R <= 0 || stride <= 0 || nwin <= 0 || W <= 0) return SNRSE_EINVAL;
  const dim3 grid((unsigned)((W + WT - 1) / WT), (unsigned)(nwin < 65535 ? nwin : 65535));
  hipLaunchKernelGGL(window_gather_kernel, grid, dim3(WT), 0, stream, src, lengths, R, stride, table, nwin, W, out);
  return (int)hipGetLastError();
}

extern "C" int snrse_window_merge(const float* win, int nwin, int W, const int* starts, const unsigned char* silent,
                                  const int* first, const int* lengths, int R, const float* fade, int V, float* out,
                                  long long stride_out, hipStream_t stream) {
  if (!win || !starts || !silent || !first || !lengths || !fade || !out) return SNRSE_EINVAL;
  if (nwin <= 0 || W <= 0 || R <= 0 || V <= 0 || stride_out <= 0 || 4LL * V > W) return SNRSE_EINVAL;
  const long long nblk = (stride_out + WT - 1) / WT;
  if (nblk > 0x7fffffffLL) return SNRSE_EINVAL;
  const dim3 grid((unsigned)nblk, (unsigned)(R < 65535 ? R : 65535));
  hipLaunchKernelGGL(window_merge_kernel, grid, dim3(WT), 0, stream, win, nwin, W, starts, silent, first, lengths, R,
                     fade, V, out, stride_out);
  return (int)hipGetLastError();
}
