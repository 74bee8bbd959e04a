// Sample-rate conversion of waveforms in front of the network (snrse.ops.resample_poly): rational polyphase FIR
// resampling of a ragged batch of fp32 rows, the arithmetic of
// scipy.signal.resample_poly(x, up, down, window=w, padtype='constant').  With up, down coprime,
// half = (len(w) - 1) / 2, h = up w and n_out = ceil(L up / down):
//   y[m] = sum_n x[n] h[m down + half - n up]     0 <= n < L,  0 <= m down + half - n up <= 2 half
// (resample.hip is the network's 2-D FIR up / down-sampling and has nothing to do with this file.)
//
// One output sample per thread, RP outputs per block.  With c = m down + half, nh = c / up and phase p = c % up the
// sum is  sum_j x[nh - j] h[p + j up],  j = 0 .. K - 1,  K = ceil((2 half + 1) / up): the taps arrive phase-major
// [up][K] (zero where p + j up > 2 half), so a thread walks its phase's taps contiguously, and the block's input
// span -- about RP down / up + K samples -- is staged in LDS with zeros outside [0, L_b).  All the guards are in
// the staging; the K-term loop has none.  The sum runs over j ascending in one fp32 fma chain: no atomics, the
// same bits on every launch, and a row's bits do not depend on the rows it shares the launch with.
// Nothing at or past L_b of a row is read; outputs [n_out_b, stride_out) are written as zero.
#include "common.h"

namespace {

constexpr int RP = 256;            // outputs per block = threads per block
constexpr int RP_MAX_SPAN = 16384;  // floats of LDS (64 KB) a block's input span may take

SNRSE_DEV long long row_len(const int* lengths, int b, long long stride_in) {
  const long long L = lengths[b];
  return L < 0 ? 0 : (L > stride_in ? stride_in : L);
}

__global__ __launch_bounds__(RP) void resample_poly_kernel(const float* __restrict__ x,
                                                           const int* __restrict__ lengths, int B,
                                                           long long stride_in, int up, int down, int half, int K,
                                                           const float* __restrict__ taps, float* __restrict__ y,
                                                           long long stride_out) {
  extern __shared__ float xs[];
  const int tid = threadIdx.x;
  const long long m0 = (long long)blockIdx.x * RP, m = m0 + tid;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_len(lengths, b, stride_in);
    long long n_out = (L * up + down - 1) / down;
    if (n_out > stride_out) n_out = stride_out;
    const float* xr = x + (size_t)b * (size_t)stride_in;
    float* yr = y + (size_t)b * (size_t)stride_out;
    if (m0 >= n_out) {  // the whole block lies in the row's zero tail (the same decision in every thread)
      if (m < stride_out) yr[m] = 0.0f;
      continue;
    }
    const long long mlast = (m0 + RP < n_out ? m0 + RP : n_out) - 1;
    const long long lo = (m0 * down + half) / up - (K - 1);
    const int span = (int)((mlast * down + half) / up - lo) + 1;
    __syncthreads();  // the previous row's readers are done with xs
    for (int i = tid; i < span; i += RP) {
      const long long n = lo + i;
      xs[i] = (n >= 0 && n < L) ? xr[n] : 0.0f;
    }
    __syncthreads();
    if (m < n_out) {
      const long long c = m * down + half, nh = c / up;
      const float* __restrict__ tp = taps + (size_t)(c - nh * up) * (size_t)K;
      const float* xp = xs + (int)(nh - lo);
      float acc = 0.0f;
      for (int j = 0; j < K; ++j) acc = fmaf(xp[-j], tp[j], acc);
      yr[m] = acc;
    } else if (m < stride_out) {
      yr[m] = 0.0f;
    }
  }
}

// up == down: the row as it is, zero from L_b on
__global__ __launch_bounds__(RP) void resample_copy_kernel(const float* __restrict__ x,
                                                           const int* __restrict__ lengths, int B,
                                                           long long stride_in, float* __restrict__ y,
                                                           long long stride_out) {
  const long long m = (long long)blockIdx.x * RP + threadIdx.x;
  if (m >= stride_out) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_len(lengths, b, stride_in);
    y[(size_t)b * (size_t)stride_out + (size_t)m] = m < L ? x[(size_t)b * (size_t)stride_in + (size_t)m] : 0.0f;
  }
}

long long gcd_ll(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

}  // namespace

extern "C" int snrse_resample_poly_block(void) { return RP; }

extern "C" int snrse_resample_poly(const float* x, const int* lengths, int B, long long stride_in, int up, int down,
                                   int half, const float* taps, float* y, long long stride_out,
                                   hipStream_t stream) {
  if (!lengths || !y || B <= 0 || stride_in < 0 || stride_out <= 0 || up <= 0 || down <= 0) return SNRSE_EINVAL;
  if (stride_in > 0 && !x) return SNRSE_EINVAL;
  if (gcd_ll(up, down) != 1) return SNRSE_EINVAL;
  const long long nblk = (stride_out + RP - 1) / RP;
  if (nblk > 0x7fffffffLL) return SNRSE_EINVAL;
  const dim3 grid((unsigned)nblk, (unsigned)(B < 65535 ? B : 65535));
  if (up == 1 && down == 1) {
    hipLaunchKernelGGL(resample_copy_kernel, grid, dim3(RP), 0, stream, x, lengths, B, stride_in, y, stride_out);
    return (int)hipGetLastError();
  }
  if (!taps || half < 0 || half > (1 << 28)) return SNRSE_EINVAL;
  const int K = (2 * half + up) / up;  // ceil((2 half + 1) / up)
  const long long span = ((long long)(RP - 1) * down) / up + K + 2;
  if (span > RP_MAX_SPAN) return SNRSE_EINVAL;
  hipLaunchKernelGGL(resample_poly_kernel, grid, dim3(RP), (size_t)span * sizeof(float), stream, x, lengths, B,
                     stride_in, up, down, half, K, taps, y, stride_out);
  return (int)hipGetLastError();
}
