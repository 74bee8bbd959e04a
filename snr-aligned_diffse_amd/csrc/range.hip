// Range statistics of a stored tensor (snrse_range_stats): per row, the largest finite magnitude and the number
// of inf / NaN elements.  The fp16 fast path packs with round-to-nearest (H16<f16_t>::pack), so a value above
// 65504 is stored as +-inf; the statistics the GEMM epilogues write are taken before the pack and cannot see
// it.  This pass looks at what was stored: the guard (snrse/guard.py) runs it once per call on the returned
// spectrogram, the range probe (NCSNppHIP.range_report) on every tensor of one evaluation.
//
// A streaming, HBM-bound reduction: grid (blocks per row, rows), so no row index is computed per element;
// 16-B loads over the 16-B aligned body of a row, scalar loads for the (at most 16 / elemsize - 1) elements
// before it and after it -- a row starts misaligned when per * elemsize % 16 != 0.  Values are classified on
// their bit patterns (exponent all ones = non-finite), and since the patterns of non-negative floats order as
// unsigned integers the peak is an integer max all the way to the one atomic a block issues.
#include <limits.h>

#include "common.h"

namespace {

constexpr int RT = 256;  // threads per block
constexpr int RU = 4;    // 16-B loads a thread keeps in flight per pass

template <int DT> struct Fmt;
template <> struct Fmt<SNRSE_F32> {
  static constexpr int kBytes = 4;
  typedef uint32_t elem_t;
  // |v| pattern of a finite peak -> f32 pattern
  SNRSE_DEV static uint32_t to_f32(uint32_t a) { return a; }
};
template <> struct Fmt<SNRSE_BF16> {
  static constexpr int kBytes = 2;
  static constexpr uint32_t kInf = 0x7f80u;
  typedef uint16_t elem_t;
  SNRSE_DEV static uint32_t to_f32(uint32_t a) { return a << 16; }
};
template <> struct Fmt<SNRSE_F16> {
  static constexpr int kBytes = 2;
  static constexpr uint32_t kInf = 0x7c00u;
  typedef uint16_t elem_t;
  // exact, whatever the denormal mode: mant * 2^-24 below the normal range, else a re-biased exponent
  SNRSE_DEV static uint32_t to_f32(uint32_t a) {
    return a < 0x0400u ? __float_as_uint((float)a * 5.9604644775390625e-8f) : (a << 13) + (112u << 23);
  }
};

// one |v| pattern: counted when its exponent is all ones, else folded into the peak
template <uint32_t kInf>
SNRSE_DEV void fold(uint32_t a, uint32_t& peak, uint32_t& bad) {
  const bool nf = a >= kInf;
  bad += nf;
  peak = max(peak, nf ? 0u : a);
}
// one 32-bit word of the row: an f32, or two 16-bit values
template <int DT>
SNRSE_DEV void fold_word(uint32_t w, uint32_t& peak, uint32_t& bad) {
  if constexpr (DT == SNRSE_F32) {
    fold<0x7f800000u>(w & 0x7fffffffu, peak, bad);
  } else {
    fold<Fmt<DT>::kInf>(w & 0x7fffu, peak, bad);
    fold<Fmt<DT>::kInf>((w >> 16) & 0x7fffu, peak, bad);
  }
}
template <int DT>
SNRSE_DEV void fold_elem(typename Fmt<DT>::elem_t e, uint32_t& peak, uint32_t& bad) {
  if constexpr (DT == SNRSE_F32)
    fold<0x7f800000u>(e & 0x7fffffffu, peak, bad);
  else
    fold<Fmt<DT>::kInf>(e & 0x7fffu, peak, bad);
}

__global__ void range_init_kernel(float* peak, int* nonfinite, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    peak[b] = 0.f;
    nonfinite[b] = 0;
  }
}

// direct: the row's only block stores its result (no fold into the slot's contents); else the slot holds a
// valid (peak >= 0, count) pair and the block folds into it with one max / one saturating add, skipped when
// they would change nothing.
template <int DT>
__global__ __launch_bounds__(RT) void range_stats_kernel(const void* __restrict__ src, int B, long long per,
                                                         float* __restrict__ peak_out, int* __restrict__ nf_out,
                                                         int direct) {
  typedef typename Fmt<DT>::elem_t elem_t;
  constexpr int ES = Fmt<DT>::kBytes, PV = 16 / ES;  // elements per 16-B vector
  const int tid = threadIdx.x;
  __shared__ uint32_t s_peak[RT / 64];
  __shared__ unsigned long long s_bad[RT / 64];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const elem_t* row = (const elem_t*)src + (size_t)b * (size_t)per;
    const uint32_t mis = (uint32_t)((uintptr_t)row & 15u);
    long long head = mis ? (16 - mis) / ES : 0;  // elements before the first 16-B boundary
    if (head > per) head = per;
    const long long nvec = (per - head) / PV;
    const long long tail0 = head + nvec * PV;  // first element after the aligned body
    const u32x4* body = (const u32x4*)(row + head);
    uint32_t pk = 0, bad = 0;  // a thread sees < 2^32 elements: per / RT of them at most
#pragma unroll RU
    for (long long i = (long long)blockIdx.x * RT + tid; i < nvec; i += (long long)gridDim.x * RT) {
      const u32x4 v = body[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) fold_word<DT>(v[k], pk, bad);
    }
    if (blockIdx.x == 0) {
      const long long nscalar = head + (per - tail0);  // < 2 PV
      for (long long i = tid; i < nscalar; i += RT) fold_elem<DT>(row[i < head ? i : tail0 + (i - head)], pk, bad);
    }
    unsigned long long nb = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      pk = max(pk, (uint32_t)__shfl_xor((int)pk, o, 64));
      nb += __shfl_xor(nb, o, 64);
    }
    if ((tid & 63) == 0) {
      s_peak[tid >> 6] = pk;
      s_bad[tid >> 6] = nb;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < RT / 64; ++w) {
        pk = max(pk, s_peak[w]);
        nb += s_bad[w];
      }
      const uint32_t pf = Fmt<DT>::to_f32(pk);
      const int cnt = nb > (unsigned long long)INT_MAX ? INT_MAX : (int)nb;
      if (direct) {
        peak_out[b] = __uint_as_float(pf);
        nf_out[b] = cnt;
      } else {
        if (pf) atomicMax((unsigned int*)peak_out + b, pf);
        if (cnt) {  // saturating add
          int old = __hip_atomic_load(nf_out + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          while (true) {
            const long long sum = (long long)old + cnt;
            const int want = sum > INT_MAX ? INT_MAX : (int)sum;
            const int seen = atomicCAS(nf_out + b, old, want);
            if (seen == old) break;
            old = seen;
          }
        }
      }
    }
    __syncthreads();  // s_peak / s_bad are reused by the next row of this block
  }
}

}  // namespace

extern "C" int snrse_range_stats(const void* src, int B, long long per, int dtype, float* peak, int* nonfinite,
                                 int accumulate, hipStream_t stream) {
  if (!src || !peak || !nonfinite || B <= 0 || per <= 0) return SNRSE_EINVAL;
  if (dtype != SNRSE_F32 && dtype != SNRSE_F16 && dtype != SNRSE_BF16) return SNRSE_EINVAL;
  const int es = dtype == SNRSE_F32 ? 4 : 2;
  if ((uintptr_t)src % es) return SNRSE_EINVAL;
  // enough blocks to fill the chip (256 CUs x 4), each thread RU vectors per pass; a block per row for small rows
  const long long nvec = per / (16 / es);
  const int rows = B < 65535 ? B : 65535;
  long long bpr = (nvec + (long long)RT * RU - 1) / ((long long)RT * RU);
  const long long cap = 1024 / rows > 1 ? 1024 / rows : 1;
  bpr = bpr < 1 ? 1 : (bpr > cap ? cap : bpr);
  const int direct = !accumulate && bpr == 1;
  if (!accumulate && !direct) {
    hipLaunchKernelGGL(range_init_kernel, dim3((B + RT - 1) / RT), dim3(RT), 0, stream, peak, nonfinite, B);
    SNRSE_LAUNCH_CHECK();
  }
  const dim3 grid((unsigned)bpr, (unsigned)rows);
  if (dtype == SNRSE_F32)
    hipLaunchKernelGGL(range_stats_kernel<SNRSE_F32>, grid, dim3(RT), 0, stream, src, B, per, peak, nonfinite, direct);
  else if (dtype == SNRSE_F16)
    hipLaunchKernelGGL(range_stats_kernel<SNRSE_F16>, grid, dim3(RT), 0, stream, src, B, per, peak, nonfinite, direct);
  else
    hipLaunchKernelGGL(range_stats_kernel<SNRSE_BF16>, grid, dim3(RT), 0, stream, src, B, per, peak, nonfinite, direct);
  return (int)hipGetLastError();
}
