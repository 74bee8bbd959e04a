// Programme loudness of a ragged batch of fp32 rows (snrse.ops.loudness / peak_oversampled / gain_to_pcm16,
// snrse/loudness.py): the ITU-R BS.1770-4 measure as include/snrse.h states it.
//
//   snrse_kweight_sums       K-weighted energy of every 100-ms sub-block of every row (f64)
//   snrse_loudness_gate      per file: 400-ms blocks from the sub-blocks of its channels, the two gates, I
//   snrse_peak_oversampled   per row max |.| of the 4x polyphase output, which is never written
//   snrse_gain_to_pcm16      one gain per row, the product as int16 (and optionally as f32)
//
// The K-weighting is a 4th-order IIR (two biquads, transposed direct form II as scipy.signal.lfilter runs them)
// whose high-pass poles lie at radius 0.995 .. 0.9988: fp64 state, and a recurrence that is serial along a row.
// The parallelism inside a row comes from the filter being linear in (state, input).  A row is cut into chunks of
// KC samples, and with A the 4 x 4 zero-input transition of one sample the state s_k at the start of chunk k obeys
//     s_0 = 0,   s_{k+1} = A^KC s_k + f_k,   f_k = the state chunk k ends in when it starts from zero.
//   1. kw_chunk_final:  one thread per chunk runs its chunk from the zero state and writes f_k.
//   2. kw_group_scan<0>: one thread per group of KS chunks folds the group's f_k from the zero state: F_g.
//      kw_row_scan:      one wave per row carries the group-start states S_{g+1} = A^(KC KS) S_g + F_g (64 F_g loaded
//                        by the lanes at a time and handed round by shuffles, every lane running the same sums).
//      kw_group_scan<1>: one thread per group repeats its fold from S_g and leaves s_k in the place of f_k.
//   3. kw_chunk_energy:  one thread per chunk runs its chunk again from s_k -- the recurrence's own values, not a
//                        run-in -- and sums z^2 up to the sub-block boundary inside the chunk and from it on
//                        (n100 >= KC: at most one boundary); two partials per chunk.
//   4. kw_fold:          one wave per sub-block adds the partials of the chunks it covers, lane l taking chunks
//                        l, l + 64, .. of the sub-block in that order, then a butterfly over the lanes.
// The filtered signal lives in registers only.  No floating-point atomics and a fixed order of every sum, all of
// them indexed from the row's own start: a row's bits do not depend on the batch, its place in it, or the launch.
//
// Passes 1 and 3 read the samples: a block stages its KT chunks (KC KT samples, one contiguous span) in LDS with
// coalesced 16-byte loads and every thread then walks its own chunk there.  A chunk's pitch in LDS is KC + 1
// words, so the 32 lanes of a half wave, KC + 1 words apart, read 32 different banks.
// Compiled without fp contraction (snrse/build.py); the fused operations are the written-out fma() calls.
#include "common.h"

namespace {

constexpr int KC = 64;            // samples per chunk
constexpr int KT = 128;           // chunks per block = threads per block of the two passes over the samples
constexpr int KS = 512;           // chunks per scan group
constexpr int KG = KC * KT;       // samples per block
constexpr int KPITCH = KC + 1;    // LDS words per chunk
constexpr int KPAR = 42;          // doubles per row of the parameter table: 10 coefficients, A^KC, A^(KC KS)

SNRSE_DEV int row_length(const int* lengths, int b, long long stride) {
  const long long L = lengths[b];
  return (int)(L < 0 ? 0 : (L > stride ? stride : L));
}

struct KW {
  double b0, b1, b2, na1, na2, h0, h1, h2, nh1, nh2;
};
SNRSE_DEV KW load_kw(const double* __restrict__ p) {
  KW c;
  c.b0 = p[0], c.b1 = p[1], c.b2 = p[2], c.na1 = -p[3], c.na2 = -p[4];
  c.h0 = p[5], c.h1 = p[6], c.h2 = p[7], c.nh1 = -p[8], c.nh2 = -p[9];
  return c;
}
// one sample through shelf then high-pass; s = (shelf w1, w2, high-pass w1, w2)
SNRSE_DEV double kw_step(const KW& c, double x, double (&s)[4]) {
  const double y = fma(c.b0, x, s[0]);
  s[0] = fma(c.b1, x, fma(c.na1, y, s[1]));
  s[1] = fma(c.b2, x, c.na2 * y);
  const double z = fma(c.h0, y, s[2]);
  s[2] = fma(c.h1, y, fma(c.nh1, z, s[3]));
  s[3] = fma(c.h2, y, c.nh2 * z);
  return z;
}
// s <- M s + f, M row-major 4 x 4
SNRSE_DEV void affine4(const double (&M)[16], const double (&f)[4], double (&s)[4]) {
  double r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] = fma(M[4 * i + 3], s[3], fma(M[4 * i + 2], s[2], fma(M[4 * i + 1], s[1], fma(M[4 * i], s[0], f[i]))));
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = r[i];
}

SNRSE_DEV int lds_idx(int i) { return i + (i >> 6); }  // i + i / KC
static_assert(KC == 64, "lds_idx shifts by log2 KC");

// samples [0, cnt) at p (4-B aligned, cnt <= KG) into xs: 16-B loads over the aligned interior, scalars at its ends
SNRSE_DEV void stage_group(const float* __restrict__ p, int cnt, float* xs) {
  const int tid = threadIdx.x;
  const int mis = (int)(((uintptr_t)p >> 2) & 3);
  int head = (4 - mis) & 3;
  if (head > cnt) head = cnt;
  const int nvec = (cnt - head) >> 2;
  const int tail0 = head + 4 * nvec;
  for (int v = tid; v < nvec; v += KT) {
    const int i = head + 4 * v;
    const f32x4 r = *(const f32x4*)(p + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[lds_idx(i + j)] = r[j];
  }
  if (tid < head) xs[lds_idx(tid)] = p[tid];
  if (tid < 4 && tail0 + tid < cnt) xs[lds_idx(tail0 + tid)] = p[tail0 + tid];
}

// pass 1.  grid (groups, rows).  states [B][nchmax][4]: f_k of every chunk that has a successor
__global__ __launch_bounds__(KT) void kw_chunk_final(const float* __restrict__ x, const int* __restrict__ lengths,
                                                      int B, long long stride, const double* __restrict__ par,
                                                      long long nchmax, double* __restrict__ states) {
  __shared__ float xs[KT * KPITCH];
  const int tid = threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const long long g0 = (long long)blockIdx.x * KG;
    const long long nch = (L + KC - 1) / KC;
    if ((long long)blockIdx.x * KT >= nch - 1) continue;  // no chunk of this group has a successor (uniform)
    const int cnt = (int)(L - g0 < KG ? L - g0 : KG);
    __syncthreads();  // the previous row's readers are done with xs
    stage_group(x + (size_t)b * (size_t)stride + g0, cnt, xs);
    __syncthreads();
    const long long k = (long long)blockIdx.x * KT + tid;
    if (k >= nch - 1) continue;  // the row's last chunk: nobody needs its final state (a full chunk otherwise)
    const KW c = load_kw(par + (size_t)b * KPAR);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const float* xp = xs + tid * KPITCH;
#pragma unroll 4
    for (int n = 0; n < KC; ++n) kw_step(c, (double)xp[n], s);
    double* o = states + ((size_t)b * (size_t)nchmax + (size_t)k) * 4;
    *(double2*)o = make_double2(s[0], s[1]);
    *(double2*)(o + 2) = make_double2(s[2], s[3]);
  }
}

// pass 2, the two per-group folds.  One thread per (group, row).  MODE 0: F_g from the zero state into gst;
// MODE 1: from S_g (gst), writing s_k over f_k.
template <int MODE>
__global__ __launch_bounds__(64) void kw_group_scan(const int* __restrict__ lengths, int B, long long stride,
                                                     const double* __restrict__ par, long long nchmax,
                                                     long long ngrmax, double* __restrict__ states,
                                                     double* __restrict__ gst) {
  const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const long long nch = (L + KC - 1) / KC;
    const long long ngr = (nch + KS - 1) / KS;
    if (g >= ngr) continue;
    if (MODE == 0 && g >= ngr - 1) continue;  // the row's last group has no successor
    double M[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) M[i] = par[(size_t)b * KPAR + 10 + i];
    double* st = states + ((size_t)b * (size_t)nchmax + (size_t)g * KS) * 4;
    double* gs = gst + ((size_t)b * (size_t)ngrmax + (size_t)g) * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (MODE == 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = gs[i];
    }
    const long long k0 = g * KS;
    const int nt = (int)(nch - k0 < KS ? nch - k0 : KS);  // chunks of this group that exist
    for (int t = 0; t < nt; ++t) {
      double f[4] = {0.0, 0.0, 0.0, 0.0};
      if (k0 + t < nch - 1) {  // f_k exists
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = st[4 * t + i];
      }
      if (MODE == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) st[4 * t + i] = s[i];
      }
      affine4(M, f, s);
    }
    if (MODE == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) gs[i] = s[i];
    }
  }
}

// pass 2, across the groups of a row.  One wave per row; gst [B][ngrmax][4] holds F_g and leaves as S_g.
__global__ __launch_bounds__(64) void kw_row_scan(const int* __restrict__ lengths, int B, long long stride,
                                                   const double* __restrict__ par, long long ngrmax,
                                                   double* __restrict__ gst) {
  const int lane = threadIdx.x;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const long long L = row_length(lengths, b, stride);
    const long long nch = (L + KC - 1) / KC;
    const long long ngr = (nch + KS - 1) / KS;
    double M[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) M[i] = par[(size_t)b * KPAR + 26 + i];
    double* gs = gst + (size_t)b * (size_t)ngrmax * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long gb = 0; gb < ngr; gb += 64) {
      const long long g = gb + lane;
      double f[4] = {0.0, 0.0, 0.0, 0.0}, mine[4] = {0.0, 0.0, 0.0, 0.0};
      if (g < ngr - 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = gs[4 * g + i];
      }
      const int m = (int)(ngr - gb < 64 ? ngr - gb : 64);
      for (int l = 0; l < m; ++l) {
        double fl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fl[i] = __shfl(f[i], l, 64);
          if (lane == l) mine[i] = s[i];
        }
        affine4(M, fl, s);
      }
      if (g < ngr) {
#pragma unroll
        for (int i = 0; i < 4; ++i) gs[4 * g + i] = mine[i];
      }
    }
  }
}

// pass 3.  partials [B][nchmax][2]: sum z^2 of chunk k before the sub-block boundary inside it, and from it on
__global__ __launch_bounds__(KT) void kw_chunk_energy(const float* __restrict__ x, const int* __restrict__ lengths,
                                                       int B, long long stride, const double* __restrict__ par,
                                                       const int* __restrict__ n100s, long long nchmax,
                                                       const double* __restrict__ states,
                                                       double* __restrict__ partials) {
  __shared__ float xs[KT * KPITCH];
  const int tid = threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const long long g0 = (long long)blockIdx.x * KG;
    if (g0 >= L) continue;  // uniform
    const int cnt = (int)(L - g0 < KG ? L - g0 : KG);
    __syncthreads();
    stage_group(x + (size_t)b * (size_t)stride + g0, cnt, xs);
    __syncthreads();
    const long long k = (long long)blockIdx.x * KT + tid;
    const long long c0 = k * KC;
    if (c0 >= L) continue;
    const int n100 = n100s[b];
    const int nv = (int)(L - c0 < KC ? L - c0 : KC);
    int n1 = nv;  // samples of the chunk before the boundary
    if (n100 >= KC) {
      const long long p = (c0 / n100 + 1) * (long long)n100;
      if (p - c0 < nv) n1 = (int)(p - c0);
    }
    const KW c = load_kw(par + (size_t)b * KPAR);
    const double* sp = states + ((size_t)b * (size_t)nchmax + (size_t)k) * 4;
    const double2 s01 = *(const double2*)sp, s23 = *(const double2*)(sp + 2);
    double s[4] = {s01.x, s01.y, s23.x, s23.y};
    const float* xp = xs + tid * KPITCH;
    double a0 = 0.0, a1 = 0.0;
    for (int n = 0; n < n1; ++n) {
      const double z = kw_step(c, (double)xp[n], s);
      a0 = fma(z, z, a0);
    }
    for (int n = n1; n < nv; ++n) {
      const double z = kw_step(c, (double)xp[n], s);
      a1 = fma(z, z, a1);
    }
    *(double2*)(partials + ((size_t)b * (size_t)nchmax + (size_t)k) * 2) = make_double2(a0, a1);
  }
}

// pass 4.  One wave per sub-block.  grid (ceil(Nmax / 4), rows), 256 threads.
__global__ __launch_bounds__(256) void kw_fold(const int* __restrict__ lengths, int B, long long stride,
                                               const int* __restrict__ n100s, long long nchmax,
                                               const double* __restrict__ partials, double* __restrict__ sums,
                                               int Nmax) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= Nmax) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const int n100 = n100s[b];
    const long long nsub = n100 >= KC ? L / n100 : 0;
    double acc = 0.0;
    if (i < nsub) {
      const long long a = i * n100, e = a + n100;
      const long long klo = a / KC, khi = (e - 1) / KC;
      const double* p = partials + (size_t)b * (size_t)nchmax * 2;
      for (long long k = klo + lane; k <= khi; k += 64) acc += (k * KC) / n100 == i ? p[2 * k] : p[2 * k + 1];
      acc = wave_sum_d(acc);
    }
    if (lane == 0) sums[(size_t)b * (size_t)Nmax + (size_t)i] = acc;
  }
}

// ---- gating.  One block per file.
constexpr int GT = 256;

// fixed-order block sum: butterfly inside each wave, the waves in ascending order; every thread gets the result
SNRSE_DEV double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
#pragma unroll
  for (int w = 1; w < GT / 64; ++w) r += sh[w];
  return r;
}
SNRSE_DEV double block_min_d(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
#pragma unroll
  for (int w = 1; w < GT / 64; ++w) r = fmin(r, sh[w]);
  return r;
}

__global__ __launch_bounds__(GT) void loudness_gate_kernel(const double* __restrict__ sums, int Nmax,
                                                           const int* __restrict__ nsub,
                                                           const int* __restrict__ n100s,
                                                           const int* __restrict__ group, int B, int G,
                                                           double* __restrict__ out_I, int* __restrict__ out_counts,
                                                           double* __restrict__ out_margin) {
  __shared__ double sh[GT / 64];
  __shared__ int s_rows[3];
  const int tid = threadIdx.x;
  for (int gi = blockIdx.x; gi < G; gi += gridDim.x) {
    __syncthreads();
    if (tid == 0) {  // the file's rows are adjacent: first row, one past the last, fewest sub-blocks among them
      int r0 = -1, r1 = -1, ns = 0x7fffffff;
      for (int b = 0; b < B; ++b)
        if (group[b] == gi) {
          if (r0 < 0) r0 = b;
          r1 = b + 1;
          int v = nsub[b];
          v = v < 0 ? 0 : (v > Nmax ? Nmax : v);
          ns = v < ns ? v : ns;
        }
      s_rows[0] = r0, s_rows[1] = r1, s_rows[2] = r0 < 0 ? 0 : ns;
    }
    __syncthreads();
    const int r0 = s_rows[0], r1 = s_rows[1];
    const int nblk = s_rows[2] >= 4 ? s_rows[2] - 3 : 0;
    const double den = r0 < 0 ? 1.0 : 4.0 * (double)n100s[r0];
    auto energy = [&](int j) {
      double e = 0.0;
      for (int r = r0; r < r1; ++r) {
        if (group[r] != gi) continue;
        const double* s = sums + (size_t)r * (size_t)Nmax + j;
        e += (((s[0] + s[1]) + s[2]) + s[3]) / den;
      }
      return e;
    };
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    // absolute gate
    double se = 0.0, mg = inf;
    int cnt = 0;
    for (int j = tid; j < nblk; j += GT) {
      const double e = energy(j);
      const double l = -0.691 + 10.0 * log10(e);
      mg = fmin(mg, fabs(l + 70.0));
      if (l > -70.0) se += e, ++cnt;
    }
    const double sum_abs = block_sum_d(se, sh);
    const int n_abs = (int)block_sum_d((double)cnt, sh);  // counts below 2^31: exact in f64
    // relative gate
    double I = -inf;
    int n_rel = 0;
    if (n_abs > 0) {
      const double gamma = -0.691 + 10.0 * log10(sum_abs / (double)n_abs) - 10.0;
      se = 0.0, cnt = 0;
      for (int j = tid; j < nblk; j += GT) {
        const double e = energy(j);
        const double l = -0.691 + 10.0 * log10(e);
        if (!(l > -70.0)) continue;
        mg = fmin(mg, fabs(l - gamma));
        if (l > gamma) se += e, ++cnt;
      }
      const double sum_rel = block_sum_d(se, sh);
      n_rel = (int)block_sum_d((double)cnt, sh);
      if (n_rel > 0) I = -0.691 + 10.0 * log10(sum_rel / (double)n_rel);
    }
    mg = block_min_d(mg, sh);
    if (tid == 0) {
      out_I[gi] = I;
      out_counts[3 * gi] = nblk, out_counts[3 * gi + 1] = n_abs, out_counts[3 * gi + 2] = n_rel;
      out_margin[gi] = mg;
    }
  }
}

// ---- oversampled peak: the arithmetic of resample_poly_kernel (audio_resample.hip) with down = 1, the output
// folded into a maximum instead of stored.  PT tiles of PR outputs per block.
constexpr int PR = 256;
constexpr int PTILES = 16;

__global__ __launch_bounds__(PR) void peak_poly_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                       int B, long long stride, int up, int half, int K,
                                                       const float* __restrict__ taps,
                                                       unsigned int* __restrict__ out) {
  extern __shared__ float ps[];
  __shared__ float s_pk[PR / 64];
  const int tid = threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const long long n_out = L * up;
    const float* xr = x + (size_t)b * (size_t)stride;
    float pk = 0.0f;
    for (int t = 0; t < PTILES; ++t) {
      const long long m0 = ((long long)blockIdx.x * PTILES + t) * PR, m = m0 + tid;
      if (m0 >= n_out) break;  // uniform
      const long long mlast = (m0 + PR < n_out ? m0 + PR : n_out) - 1;
      const long long lo = (m0 + half) / up - (K - 1);
      const int span = (int)((mlast + half) / up - lo) + 1;
      __syncthreads();
      for (int i = tid; i < span; i += PR) {
        const long long n = lo + i;
        ps[i] = (n >= 0 && n < L) ? xr[n] : 0.0f;
      }
      __syncthreads();
      if (m < n_out) {
        const long long c = m + half, nh = c / up;
        const float* __restrict__ tp = taps + (size_t)(c - nh * up) * (size_t)K;
        const float* xp = ps + (int)(nh - lo);
        float acc = 0.0f;
        for (int j = 0; j < K; ++j) acc = fmaf(xp[-j], tp[j], acc);
        pk = fmaxf(pk, fabsf(acc));  // a NaN is skipped, as snrse_absmax skips it
      }
    }
    pk = wave_max(pk);
    __syncthreads();
    if ((tid & 63) == 0) s_pk[tid >> 6] = pk;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < PR / 64; ++w) pk = fmaxf(pk, s_pk[w]);
      // non-negative floats order as their bit patterns: an integer maximum, which commutes
      if (pk > 0.0f) atomicMax(out + b, __float_as_uint(pk));
    }
  }
}

// ---- gain and 16-bit conversion
SNRSE_DEV short to_pcm16(float v) {
  const float r = rintf(v * 32768.0f);
  return (short)(int)fminf(fmaxf(r, -32768.0f), 32767.0f);
}

constexpr int QT = 256;
__global__ __launch_bounds__(QT) void gain_to_pcm16_kernel(const float* __restrict__ x,
                                                           const int* __restrict__ lengths, int B, long long stride,
                                                           const double* __restrict__ gain, short* __restrict__ q,
                                                           float* __restrict__ f) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const size_t off = (size_t)b * (size_t)stride;
    const float* xr = x + off;
    short* qr = q + off;
    float* fr = f ? f + off : nullptr;
    const float gf = (float)gain[b];
    const bool vec = (((uintptr_t)xr | (uintptr_t)fr) & 15) == 0 && ((uintptr_t)qr & 7) == 0;
    const long long nvec = vec ? stride / 4 : 0;
    for (long long v = (long long)blockIdx.x * QT + threadIdx.x; v < nvec; v += (long long)gridDim.x * QT) {
      const long long i = 4 * v;
      f32x4 y = {0.f, 0.f, 0.f, 0.f};
      if (i < L) {
        if (i + 4 <= L) {
          const f32x4 r = *(const f32x4*)(xr + i);
#pragma unroll
          for (int j = 0; j < 4; ++j) y[j] = gf * r[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j < L) y[j] = gf * xr[i + j];
        }
      }
      if (fr) *(f32x4*)(fr + i) = y;
      uint2 w;
      w.x = (uint32_t)(uint16_t)to_pcm16(y[0]) | ((uint32_t)(uint16_t)to_pcm16(y[1]) << 16);
      w.y = (uint32_t)(uint16_t)to_pcm16(y[2]) | ((uint32_t)(uint16_t)to_pcm16(y[3]) << 16);
      *(uint2*)(qr + i) = w;
    }
    for (long long i = 4 * nvec + (long long)blockIdx.x * QT + threadIdx.x; i < stride;
         i += (long long)gridDim.x * QT) {
      const float y = i < L ? gf * xr[i] : 0.0f;
      if (fr) fr[i] = y;
      qr[i] = to_pcm16(y);
    }
  }
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct KwLayout {
  long long nchmax, nblkmax, ngrmax;
  size_t states, gst, partials, total;
};
KwLayout kw_layout(int B, long long stride) {
  KwLayout w;
  w.nchmax = (stride + KC - 1) / KC;
  w.nblkmax = (w.nchmax + KT - 1) / KT;
  w.ngrmax = (w.nchmax + KS - 1) / KS;
  w.states = 0;
  w.gst = w.states + align256((size_t)B * (size_t)w.nchmax * 4 * sizeof(double));
  w.partials = w.gst + align256((size_t)B * (size_t)w.ngrmax * 4 * sizeof(double));
  w.total = w.partials + align256((size_t)B * (size_t)w.nchmax * 2 * sizeof(double));
  return w;
}

}  // namespace

extern "C" int snrse_kweight_chunk(void) { return KC; }
extern "C" int snrse_kweight_block(void) { return KT; }
extern "C" int snrse_kweight_group(void) { return KS; }

extern "C" size_t snrse_kweight_workspace(int B, long long stride) {
  if (B <= 0 || stride <= 0 || stride > 0x7fffffffLL) return 0;
  return kw_layout(B, stride).total;
}

extern "C" int snrse_kweight_sums(const float* x, const int* lengths, int B, long long stride, const double* params,
                                  const int* n100, void* work, size_t work_bytes, double* sums, int Nmax,
                                  hipStream_t stream) {
  if (!x || !lengths || !params || !n100 || !work || !sums || B <= 0 || stride <= 0 || Nmax <= 0)
    return SNRSE_EINVAL;
  if (stride > 0x7fffffffLL || !aligned4(x) || ((uintptr_t)work & 255)) return SNRSE_EINVAL;
  const KwLayout w = kw_layout(B, stride);
  if (work_bytes < w.total) return SNRSE_EINVAL;
  double* states = (double*)((char*)work + w.states);
  double* gst = (double*)((char*)work + w.gst);
  double* partials = (double*)((char*)work + w.partials);
  const unsigned rows = (unsigned)(B < 65535 ? B : 65535);
  const dim3 ggrid((unsigned)w.nblkmax, rows);
  const dim3 sgrid((unsigned)((w.ngrmax + 63) / 64), rows);
  hipLaunchKernelGGL(kw_chunk_final, ggrid, dim3(KT), 0, stream, x, lengths, B, stride, params, w.nchmax, states);
  hipLaunchKernelGGL(kw_group_scan<0>, sgrid, dim3(64), 0, stream, lengths, B, stride, params, w.nchmax, w.ngrmax,
                     states, gst);
  hipLaunchKernelGGL(kw_row_scan, dim3((unsigned)B), dim3(64), 0, stream, lengths, B, stride, params, w.ngrmax, gst);
  hipLaunchKernelGGL(kw_group_scan<1>, sgrid, dim3(64), 0, stream, lengths, B, stride, params, w.nchmax, w.ngrmax,
                     states, gst);
  hipLaunchKernelGGL(kw_chunk_energy, ggrid, dim3(KT), 0, stream, x, lengths, B, stride, params, n100, w.nchmax,
                     states, partials);
  hipLaunchKernelGGL(kw_fold, dim3((unsigned)((Nmax + 3) / 4), rows), dim3(256), 0, stream, lengths, B, stride, n100,
                     w.nchmax, partials, sums, Nmax);
  return (int)hipGetLastError();
}

extern "C" int snrse_loudness_gate(const double* sums, int Nmax, const int* nsub, const int* n100, const int* group,
                                   int B, int G, double* out_lufs, int* out_counts, double* out_margin,
                                   hipStream_t stream) {
  if (!sums || !nsub || !n100 || !group || !out_lufs || !out_counts || !out_margin || B <= 0 || G <= 0 || Nmax <= 0)
    return SNRSE_EINVAL;
  hipLaunchKernelGGL(loudness_gate_kernel, dim3((unsigned)(G < 65535 ? G : 65535)), dim3(GT), 0, stream, sums, Nmax,
                     nsub, n100, group, B, G, out_lufs, out_counts, out_margin);
  return (int)hipGetLastError();
}

extern "C" int snrse_peak_oversampled(const float* x, const int* lengths, int B, long long stride, int up, int half,
                                      const float* taps, float* out, hipStream_t stream) {
  if (!x || !lengths || !taps || !out || B <= 0 || stride <= 0 || up < 2 || half < 0 || half > (1 << 20))
    return SNRSE_EINVAL;
  if (stride > 0x7fffffffLL / up) return SNRSE_EINVAL;
  const int K = (2 * half + up) / up;
  const long long span = (long long)(PR - 1) / up + K + 2;
  if (span > 16384) return SNRSE_EINVAL;
  SNRSE_RET(hipMemsetAsync(out, 0, (size_t)B * sizeof(float), stream));
  const long long per = (long long)PR * PTILES;
  const long long nblk = (stride * up + per - 1) / per;
  const dim3 grid((unsigned)nblk, (unsigned)(B < 65535 ? B : 65535));
  hipLaunchKernelGGL(peak_poly_kernel, grid, dim3(PR), (size_t)span * sizeof(float), stream, x, lengths, B, stride,
                     up, half, K, taps, (unsigned int*)out);
  return (int)hipGetLastError();
}

extern "C" int snrse_gain_to_pcm16(const float* x, const int* lengths, int B, long long stride, const double* gain,
                                   short* q, float* f, hipStream_t stream) {
  if (!x || !lengths || !gain || !q || B <= 0 || stride <= 0 || stride > 0x7fffffffLL) return SNRSE_EINVAL;
  if (!aligned4(x) || !aligned4(f) || ((uintptr_t)q & 1)) return SNRSE_EINVAL;
  long long bpr = (stride / 4 + (long long)QT * 4 - 1) / ((long long)QT * 4);
  const int rows = B < 65535 ? B : 65535;
  const long long cap = 2048 / rows > 1 ? 2048 / rows : 1;
  bpr = bpr < 1 ? 1 : (bpr > cap ? cap : bpr);
  hipLaunchKernelGGL(gain_to_pcm16_kernel, dim3((unsigned)bpr, (unsigned)rows), dim3(QT), 0, stream, x, lengths, B,
                     stride, gain, q, f);
  return (int)hipGetLastError();
}
