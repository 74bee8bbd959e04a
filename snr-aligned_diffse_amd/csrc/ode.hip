// Stage kernels of the per-row adaptive RK45 (snrse/ode.py rk45_solve_rows): every row of a batch integrates its
// own ODE with its own step size, so the per-element work of one attempted step is
//   snrse_rk45_combine  out[b][e] = y[b][e] + h[b] * (sum_s c_s K_s[b][e])          (5 stage states + y_new)
//   snrse_rk45_rownorm  sqrt(mean_e |m[b] sum_s c_s V_s[b][e]|^2 / scale[b][e]^2)   (error norm, initial-step norms)
//   snrse_rk45_accept   y[b] <- y_new[b], f[b] <- f_new[b] where mask[b]            (per-row accept)
// and the controller (accept / reject, next h) stays on the host in float64.
//
// All arithmetic is fp64 and every product and sum rounds on its own (no fma contraction: the pragma below and
// -ffp-contract=off in snrse/build.py), so a result is the one numpy / torch compute with the same operation
// order.  A complex state is pairs of reals: a row is n doubles, n even when complex.  K is float32 (the
// network's complex64 drift, promoted in the load) or float64.
//
// Streaming, HBM-bound kernels in range.hip's shape: grid (blocks per row, rows), size_t offsets, 16-B loads over
// the body of a row that starts at a multiple of 4 elements of the whole buffer (so a float32 K vector is 16-B
// aligned too), scalar handling of the at most 3 elements before it and after it.  The buffers' base addresses
// must be 16-B aligned.
#pragma clang fp contract(off)

#include "common.h"

namespace {

constexpr int OT = 256;    // threads per block
constexpr int OV = 4;      // elements per thread and pass: 2 x 16 B of doubles, 16 B of floats
constexpr int OMAXS = 7;   // stages of the Dormand-Prince tableau, FSAL included

typedef __attribute__((ext_vector_type(2))) double f64x2;

// stage tensors and their coefficients, by value (zero coefficients are dropped by the caller)
struct Stages {
  const void* k[OMAXS];
  double c[OMAXS];
  int ns;
};

template <bool F32>
SNRSE_DEV void load4(const void* base, size_t g, double* v) {
  if constexpr (F32) {
    const f32x4 t = *(const f32x4*)((const float*)base + g);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (double)t[k];
  } else {
    const f64x2 a = *(const f64x2*)((const double*)base + g);
    const f64x2 b = *(const f64x2*)((const double*)base + g + 2);
    v[0] = a[0];
    v[1] = a[1];
    v[2] = b[0];
    v[3] = b[1];
  }
}
template <bool F32>
SNRSE_DEV double load1(const void* base, size_t g) {
  if constexpr (F32)
    return (double)((const float*)base)[g];
  else
    return ((const double*)base)[g];
}

// sum_s c_s K_s in stage order, the first term taken as it is (snrse/ode.py _lincomb)
template <bool F32>
SNRSE_DEV void lincomb4(const Stages& st, size_t g, double* acc) {
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = 0.0;
#pragma unroll
  for (int s = 0; s < OMAXS; ++s) {
    if (s < st.ns) {
      double v[4];
      load4<F32>(st.k[s], g, v);
      const double c = st.c[s];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = s == 0 ? c * v[k] : acc[k] + c * v[k];
    }
  }
}
template <bool F32>
SNRSE_DEV double lincomb1(const Stages& st, size_t g) {
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < OMAXS; ++s) {
    if (s < st.ns) {
      const double v = load1<F32>(st.k[s], g), c = st.c[s];
      acc = s == 0 ? c * v : acc + c * v;
    }
  }
  return acc;
}

// the split of row b of n elements at offset off = b n of the buffer: [0, head) scalar, nvec vectors of OV
// elements from head on, [tail0, n) scalar
struct RowSplit {
  long long head, nvec, tail0;
};
SNRSE_DEV RowSplit split_row(size_t off, long long n) {
  RowSplit r;
  r.head = (long long)((OV - off % OV) % OV);
  if (r.head > n) r.head = n;
  r.nvec = (n - r.head) / OV;
  r.tail0 = r.head + r.nvec * OV;
  return r;
}

template <bool F32>
__global__ __launch_bounds__(OT) void combine_kernel(const double* __restrict__ y, const double* __restrict__ h,
                                                     Stages st, int B, long long n, double* __restrict__ out,
                                                     float* __restrict__ out32) {
  const int tid = threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const size_t off = (size_t)b * (size_t)n;
    const double hb = h[b];
    const RowSplit rs = split_row(off, n);
    for (long long i = (long long)blockIdx.x * OT + tid; i < rs.nvec; i += (long long)gridDim.x * OT) {
      const size_t g = off + (size_t)(rs.head + i * OV);
      double yv[4], acc[4], o[4];
      load4<false>(y, g, yv);
      lincomb4<F32>(st, g, acc);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = yv[k] + hb * acc[k];
      *(f64x2*)(out + g) = f64x2{o[0], o[1]};
      *(f64x2*)(out + g + 2) = f64x2{o[2], o[3]};
      if (out32) *(f32x4*)(out32 + g) = f32x4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
    }
    if (blockIdx.x == 0) {
      const long long nscalar = rs.head + (n - rs.tail0);  // < 2 OV
      for (long long i = tid; i < nscalar; i += OT) {
        const size_t g = off + (size_t)(i < rs.head ? i : rs.tail0 + (i - rs.head));
        const double o = y[g] + hb * lincomb1<F32>(st, g);
        out[g] = o;
        if (out32) out32[g] = (float)o;
      }
    }
  }
}

// one real element, or one complex one (vr, vi), of the scaled norm
SNRSE_DEV double term_real(double v, double a, double b2, double rtol, double atol) {
  const double q = v / (atol + rtol * fmax(fabs(a), fabs(b2)));
  return q * q;
}
SNRSE_DEV double term_cplx(double vr, double vi, double ar, double ai, double br, double bi, double rtol,
                           double atol) {
  const double s = atol + rtol * fmax(sqrt(ar * ar + ai * ai), sqrt(br * br + bi * bi));
  const double qr = vr / s, qi = vi / s;
  return qr * qr + qi * qi;
}

// pass 1: partial[b][blockIdx.x] = this block's share of sum_e |m[b] sum_s c_s V_s|^2 / scale^2
template <bool F32, bool CPLX>
__global__ __launch_bounds__(OT) void rownorm_partial_kernel(Stages st, const double* __restrict__ m,
                                                             const double* __restrict__ a,
                                                             const double* __restrict__ b2, double rtol, double atol,
                                                             int B, long long n, double* __restrict__ partial) {
  const int tid = threadIdx.x;
  __shared__ double s_sum[OT / 64];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const size_t off = (size_t)b * (size_t)n;
    const double mb = m ? m[b] : 1.0;
    const RowSplit rs = split_row(off, n);
    double sum = 0.0;
    for (long long i = (long long)blockIdx.x * OT + tid; i < rs.nvec; i += (long long)gridDim.x * OT) {
      const size_t g = off + (size_t)(rs.head + i * OV);
      double v[4], av[4], bv[4];
      lincomb4<F32>(st, g, v);
      load4<false>(a, g, av);
      load4<false>(b2, g, bv);
      if (m) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = mb * v[k];
      }
      if constexpr (CPLX) {
        sum = sum + term_cplx(v[0], v[1], av[0], av[1], bv[0], bv[1], rtol, atol);
        sum = sum + term_cplx(v[2], v[3], av[2], av[3], bv[2], bv[3], rtol, atol);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) sum = sum + term_real(v[k], av[k], bv[k], rtol, atol);
      }
    }
    if (blockIdx.x == 0) {
      // complex rows: n, off and so head and the tail are even, a pair is never split
      constexpr int step = CPLX ? 2 : 1;
      const long long nscalar = rs.head + (n - rs.tail0);
      for (long long i = (long long)tid * step; i < nscalar; i += (long long)OT * step) {
        const size_t g = off + (size_t)(i < rs.head ? i : rs.tail0 + (i - rs.head));
        double v0 = lincomb1<F32>(st, g);
        if (m) v0 = mb * v0;
        if constexpr (CPLX) {
          double v1 = lincomb1<F32>(st, g + 1);
          if (m) v1 = mb * v1;
          sum = sum + term_cplx(v0, v1, a[g], a[g + 1], b2[g], b2[g + 1], rtol, atol);
        } else {
          sum = sum + term_real(v0, a[g], b2[g], rtol, atol);
        }
      }
    }
    sum = wave_sum_d(sum);
    if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < OT / 64; ++w) sum = sum + s_sum[w];
      partial[(size_t)b * gridDim.x + blockIdx.x] = sum;
    }
    __syncthreads();  // s_sum is reused by the next row of this block
  }
}

// pass 2: the row's partials folded in block order by one thread, out[b] = sqrt(sum / count)
__global__ void rownorm_fold_kernel(const double* __restrict__ partial, int B, int bpr, double count,
                                    double* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double sum = 0.0;
  for (int k = 0; k < bpr; ++k) sum = sum + partial[(size_t)b * bpr + k];
  out[b] = sqrt(sum / count);
}

// dst[off, off + w) <- src[off, off + w) in 32-bit words, 16-B vectors over the aligned body
SNRSE_DEV void copy_row(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, size_t off, long long w,
                        int tid) {
  const RowSplit rs = split_row(off, w);
  for (long long i = (long long)blockIdx.x * OT + tid; i < rs.nvec; i += (long long)gridDim.x * OT) {
    const size_t g = off + (size_t)(rs.head + i * OV);
    *(u32x4*)(dst + g) = *(const u32x4*)(src + g);
  }
  if (blockIdx.x == 0) {
    const long long nscalar = rs.head + (w - rs.tail0);
    for (long long i = tid; i < nscalar; i += OT) {
      const size_t g = off + (size_t)(i < rs.head ? i : rs.tail0 + (i - rs.head));
      dst[g] = src[g];
    }
  }
}

__global__ __launch_bounds__(OT) void accept_kernel(const int* __restrict__ mask, uint32_t* __restrict__ y,
                                                    const uint32_t* __restrict__ y_new, long long wy,
                                                    uint32_t* __restrict__ f, const uint32_t* __restrict__ f_new,
                                                    long long wf, int B) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    if (!mask[b]) continue;
    copy_row(y, y_new, (size_t)b * (size_t)wy, wy, threadIdx.x);
    copy_row(f, f_new, (size_t)b * (size_t)wf, wf, threadIdx.x);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// blocks per row: each thread a few vectors per pass, about 1024 blocks over the rows at most
int blocks_per_row(int B, long long n) {
  const int rows = B < 65535 ? B : 65535;
  long long bpr = (n / OV + (long long)OT * 4 - 1) / ((long long)OT * 4);
  const long long cap = 1024 / rows > 1 ? 1024 / rows : 1;
  return (int)(bpr < 1 ? 1 : (bpr > cap ? cap : bpr));
}

// host arrays (k, c, ns) -> Stages; false when a pointer is null or misaligned
bool make_stages(const void* const* k, const double* c, int ns, Stages& st) {
  if (ns < 0 || ns > OMAXS || (ns > 0 && (!k || !c))) return false;
  st.ns = ns;
  for (int s = 0; s < OMAXS; ++s) {
    st.k[s] = s < ns ? k[s] : nullptr;
    st.c[s] = s < ns ? c[s] : 0.0;
    if (s < ns && (!k[s] || !aligned16(k[s]))) return false;
  }
  return true;
}

}  // namespace

extern "C" int snrse_rk45_rownorm_blocks(int B, long long n) {
  return (B <= 0 || n <= 0) ? 0 : blocks_per_row(B, n);
}

extern "C" int snrse_rk45_combine(const double* y, const double* h, const void* const* k, const double* c, int ns,
                                  int kdtype, int B, long long n, double* out, float* out32, hipStream_t stream) {
  Stages st;
  if (!y || !h || !out || B <= 0 || n <= 0 || !make_stages(k, c, ns, st)) return SNRSE_EINVAL;
  if (kdtype != SNRSE_F32 && kdtype != SNRSE_F64) return SNRSE_EINVAL;
  if (!aligned16(y) || !aligned16(out) || !aligned16(out32) || ((uintptr_t)h & 7u)) return SNRSE_EINVAL;
  const dim3 grid((unsigned)blocks_per_row(B, n), (unsigned)(B < 65535 ? B : 65535));
  if (kdtype == SNRSE_F32)
    hipLaunchKernelGGL(combine_kernel<true>, grid, dim3(OT), 0, stream, y, h, st, B, n, out, out32);
  else
    hipLaunchKernelGGL(combine_kernel<false>, grid, dim3(OT), 0, stream, y, h, st, B, n, out, out32);
  return (int)hipGetLastError();
}

extern "C" int snrse_rk45_rownorm(const void* const* v, const double* c, int ns, int vdtype, const double* m,
                                  const double* a, const double* b2, double rtol, double atol, int cplx, int B,
                                  long long n, double* partial, double* out, hipStream_t stream) {
  Stages st;
  if (!a || !b2 || !partial || !out || B <= 0 || n <= 0 || !make_stages(v, c, ns, st)) return SNRSE_EINVAL;
  if (vdtype != SNRSE_F32 && vdtype != SNRSE_F64) return SNRSE_EINVAL;
  if (cplx && (n & 1)) return SNRSE_EINVAL;
  if (!aligned16(a) || !aligned16(b2) || ((uintptr_t)m & 7u) || ((uintptr_t)partial & 7u) || ((uintptr_t)out & 7u))
    return SNRSE_EINVAL;
  const int bpr = blocks_per_row(B, n);
  const dim3 grid((unsigned)bpr, (unsigned)(B < 65535 ? B : 65535));
  const bool f32 = vdtype == SNRSE_F32;
  if (f32 && cplx)
    hipLaunchKernelGGL((rownorm_partial_kernel<true, true>), grid, dim3(OT), 0, stream, st, m, a, b2, rtol, atol, B, n,
                       partial);
  else if (f32)
    hipLaunchKernelGGL((rownorm_partial_kernel<true, false>), grid, dim3(OT), 0, stream, st, m, a, b2, rtol, atol, B,
                       n, partial);
  else if (cplx)
    hipLaunchKernelGGL((rownorm_partial_kernel<false, true>), grid, dim3(OT), 0, stream, st, m, a, b2, rtol, atol, B,
                       n, partial);
  else
    hipLaunchKernelGGL((rownorm_partial_kernel<false, false>), grid, dim3(OT), 0, stream, st, m, a, b2, rtol, atol, B,
                       n, partial);
  SNRSE_LAUNCH_CHECK();
  const double count = cplx ? (double)(n / 2) : (double)n;
  hipLaunchKernelGGL(rownorm_fold_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, partial, B, bpr, count, out);
  return (int)hipGetLastError();
}

extern "C" int snrse_rk45_accept(const int* mask, void* y, const void* y_new, long long ywords, void* f,
                                 const void* f_new, long long fwords, int B, hipStream_t stream) {
  if (!mask || !y || !y_new || !f || !f_new || B <= 0 || ywords <= 0 || fwords <= 0) return SNRSE_EINVAL;
  if (!aligned16(y) || !aligned16(y_new) || !aligned16(f) || !aligned16(f_new) || ((uintptr_t)mask & 3u))
    return SNRSE_EINVAL;
  const long long w = ywords > fwords ? ywords : fwords;
  const dim3 grid((unsigned)blocks_per_row(B, w), (unsigned)(B < 65535 ? B : 65535));
  hipLaunchKernelGGL(accept_kernel, grid, dim3(OT), 0, stream, mask, (uint32_t*)y, (const uint32_t*)y_new, ywords,
                     (uint32_t*)f, (const uint32_t*)f_new, fwords, B);
  return (int)hipGetLastError();
}
