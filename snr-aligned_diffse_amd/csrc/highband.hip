// The band above the network's 8 kHz, kept at the recording's own rate R > 16 kHz (snrse.ops.band_gain,
// snrse.ops.resample_mix; the definition stands in include/snrse.h).  With y the recording at rate R, u its 16 kHz
// version, x the enhanced 16 kHz row, h the 16 k -> R filter and U(v)[n] = sum_j v[j] h[n down + half - j up]
// (snrse_resample_poly's arithmetic):
//   out[n] = U(x)[n] + g[n] (y[n] - U(u)[n]) = g[n] y[n] + sum_j h[.] (x[j] - g[n] u[j])
//
// snrse_resample_mix is that sum in audio_resample.hip's layout: one output per thread, HP outputs per block, the
// taps phase-major, the block's span of x and u staged in LDS as (x, u) pairs with zeros outside [0, L16_b), all the
// guards in the staging.  Per output, every operation written out (the file is built with -ffp-contract=off):
//   a  = fl(rem / den), om = fl((den - rem) / den)    divided in fp64, rounded to fp32 once each
//   g  = fma(a, g1, fl(om g0))                        <= 3 roundings relative to g (g0, g1 >= 0: no cancellation)
//   d_j = fma(-g, u_j, x_j)                           1 rounding
//   acc = fma(d_j, h_j, acc), j ascending             <= K roundings per term
//   out = fma(g, y, acc)                              1 rounding
// so a g|u_j||h_j| term carries at most K + 5 roundings, an |x_j||h_j| term K + 2 and g|y| 4: inside the
// (K + 8) 2^-24 (g|y| + sum_j |h_j| (|x_j| + g|u_j|)) the tests hold it to.  With g = 1 and x = u every d_j is an
// exact zero and out = y bit for bit.  No atomics, one summation order, a row's bits do not depend on its batch.
//
// snrse_band_gain is the "follow" policy's gain track: the energies of bins 128 .. 255 of the raw STFT (n_fft 510,
// hop 128, periodic Hann, centred, reflect at the row's own L16) of u and of x, their clamped ratio per frame and
// its truncated 5-frame mean.  The DFT, the energies and the ratios are fp64 (the gain is a ratio of two sums of
// 128 squares: in fp32 its error would be the front end's, not the definition's); the result is rounded to fp32
// once.  Two kernels on the caller's stream, the energies passing through a caller's workspace: no host
// synchronisation, fixed summation orders.
#include "common.h"

namespace {

constexpr int HP = 256;             // outputs per block = threads per block (snrse_resample_poly's)
constexpr int HP_MAX_SPAN = 16384;  // floats of LDS (64 KB) a block's staged input may take, x and u together

constexpr int NFFT = 510;
constexpr int HOP = 128;
constexpr int BIN0 = 128;  // first bin of the top octave
constexpr int NB = 128;    // bins 128 .. 255
constexpr int FPB = 8;     // frames per block
constexpr int BSPAN = (FPB - 1) * HOP + NFFT;

SNRSE_DEV long long clamp_len(const int* lengths, int b, long long stride) {
  const long long L = lengths[b];
  return L < 0 ? 0 : (L > stride ? stride : L);
}

__global__ __launch_bounds__(HP) void resample_mix_kernel(
    const float* __restrict__ x, const float* __restrict__ u, const int* __restrict__ len16, long long stride16,
    const float* __restrict__ y, const int* __restrict__ lenR, long long strideR, int B, int up, int down, int half,
    int K, const float* __restrict__ taps, const float* __restrict__ gains, const int* __restrict__ frames, int Tmax,
    float gain_const, float* __restrict__ out) {
  extern __shared__ float2 xu[];  // (x, u) pairs of the block's input span
  const int tid = threadIdx.x;
  const long long m0 = (long long)blockIdx.x * HP, m = m0 + tid;
  const long long den = (long long)up * HOP;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L16 = clamp_len(len16, b, stride16);
    const long long L = clamp_len(lenR, b, strideR);
    float* outr = out + (size_t)b * (size_t)strideR;
    if (m0 >= L) {  // the whole block lies in the row's zero tail (the same decision in every thread)
      if (m < strideR) outr[m] = 0.0f;
      continue;
    }
    const float* xr = x + (size_t)b * (size_t)stride16;
    const float* ur = u + (size_t)b * (size_t)stride16;
    const long long mlast = (m0 + HP < L ? m0 + HP : L) - 1;
    const long long lo = (m0 * down + half) / up - (K - 1);
    const int span = (int)((mlast * down + half) / up - lo) + 1;
    __syncthreads();  // the previous row's readers are done with xu
    for (int i = tid; i < span; i += HP) {
      const long long n = lo + i;
      const bool in = n >= 0 && n < L16;
      xu[i] = make_float2(in ? xr[n] : 0.0f, in ? ur[n] : 0.0f);
    }
    __syncthreads();
    if (m < L) {
      float g = gain_const;
      if (gains) {
        int T = frames[b];
        T = T > Tmax ? Tmax : T;
        g = 0.0f;
        if (T > 0) {  // frame centre i sits at output sample i 128 up / down
          const long long num = m * down, i = num / den, rem = num - i * den;
          const float* gr = gains + (size_t)b * (size_t)Tmax;
          const float g0 = gr[i < T - 1 ? i : T - 1], g1 = gr[i + 1 < T - 1 ? i + 1 : T - 1];
          const float a = (float)((double)rem / (double)den), om = (float)((double)(den - rem) / (double)den);
          g = fmaf(a, g1, om * g0);
        }
      }
      const long long c = m * down + half, nh = c / up;
      const float* __restrict__ tp = taps + (size_t)(c - nh * up) * (size_t)K;
      const float2* p = xu + (int)(nh - lo);
      float acc = 0.0f;
      for (int j = 0; j < K; ++j) {
        const float2 v = p[-j];
        acc = fmaf(fmaf(-g, v.y, v.x), tp[j], acc);
      }
      outr[m] = fmaf(g, y[(size_t)b * (size_t)strideR + (size_t)m], acc);
    } else if (m < strideR) {
      outr[m] = 0.0f;
    }
  }
}

// energies [B][2][Tmax] f64: (b, 0, t) the top-octave energy of frame t of u, (b, 1, t) of x; frames at or past
// T_b = 1 + L_b / 128 are not written.  Threads 0 .. 127 take bins 128 .. 255 of u, threads 128 .. 255 those of x.
__global__ __launch_bounds__(256) void band_energy_kernel(const float* __restrict__ u, const float* __restrict__ x,
                                                          const int* __restrict__ lengths, int Lstride, int Tmax,
                                                          double* __restrict__ energies) {
  __shared__ double cs[NFFT], sn[NFFT];
  __shared__ double xs[2][BSPAN];
  __shared__ double red[FPB][2 * NB];
  const int b = blockIdx.y, f0 = blockIdx.x * FPB, tid = threadIdx.x;
  const int L = min(max(lengths[b], 1), Lstride);
  const int T = min(1 + L / HOP, Tmax);
  if (f0 >= T) return;  // the same decision in every thread
  for (int m = tid; m < NFFT; m += 256) {
    double s, c;
    sincospi(2.0 * (double)m / NFFT, &s, &c);
    cs[m] = c;
    sn[m] = s;
  }
  for (int j = tid; j < BSPAN; j += 256) {
    int s = f0 * HOP + j - NFFT / 2;
    if (s < 0) s = -s;
    if (s >= L) s = 2 * (L - 1) - s;
    // frames >= T_b read past the reflect range (their energies are dropped), and so does a row too short to
    // reflect, which the host refuses: the clamp keeps every address inside [0, L_b)
    s = s < 0 ? 0 : (s >= L ? L - 1 : s);
    xs[0][j] = (double)u[(size_t)b * Lstride + s];
    xs[1][j] = (double)x[(size_t)b * Lstride + s];
  }
  __syncthreads();
  const int sig = tid >> 7, k = BIN0 + (tid & (NB - 1));
  const double* xv = xs[sig];
  double re[FPB], im[FPB];
#pragma unroll
  for (int f = 0; f < FPB; ++f) re[f] = im[f] = 0.0;
  int idx = 0;  // (k n) mod 510
  for (int n = 0; n < NFFT; ++n) {
    const double w = 0.5 - 0.5 * cs[n];  // periodic Hann
    const double c = cs[idx], s = sn[idx];
#pragma unroll
    for (int f = 0; f < FPB; ++f) {
      const double v = xv[f * HOP + n] * w;
      re[f] = fma(v, c, re[f]);
      im[f] = fma(-v, s, im[f]);
    }
    idx += k;
    if (idx >= NFFT) idx -= NFFT;
  }
#pragma unroll
  for (int f = 0; f < FPB; ++f) red[f][tid] = fma(re[f], re[f], im[f] * im[f]);
  __syncthreads();
  if (tid < 2 * FPB) {  // one thread per (frame, signal): the 128 bins in ascending order
    const int f = tid >> 1, s = tid & 1;
    double e = 0.0;
    for (int i = 0; i < NB; ++i) e += red[f][s * NB + i];
    if (f0 + f < T) energies[((size_t)b * 2 + s) * Tmax + f0 + f] = e;
  }
}

// gains [B][Tmax] f32: the mean over frames max(0, t - 2) .. min(T_b - 1, t + 2), ascending, of
// g_f = 1 where E_u = 0, else clamp(sqrt(E_x / E_u), floor_gain, 1); zero from T_b on
__global__ __launch_bounds__(256) void band_gain_kernel(const double* __restrict__ energies,
                                                        const int* __restrict__ lengths, int B, int Lstride, int Tmax,
                                                        double floor_gain, float* __restrict__ gains) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Tmax) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int L = min(max(lengths[b], 1), Lstride);
    const int T = min(1 + L / HOP, Tmax);
    float g = 0.0f;
    if (t < T) {
      const double* eu = energies + (size_t)b * 2 * Tmax;
      const double* ex = eu + Tmax;
      const int t0 = t - 2 > 0 ? t - 2 : 0, t1 = t + 2 < T - 1 ? t + 2 : T - 1;
      double sum = 0.0;
      for (int i = t0; i <= t1; ++i) {
        double gf = 1.0;
        if (eu[i] != 0.0) {
          gf = sqrt(ex[i] / eu[i]);
          gf = gf < floor_gain ? floor_gain : (gf > 1.0 ? 1.0 : gf);
        }
        sum += gf;
      }
      g = (float)(sum / (double)(t1 - t0 + 1));
    }
    gains[(size_t)b * Tmax + t] = g;
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

extern "C" int snrse_resample_mix(const float* x, const float* u, const int* len16, long long stride16,
                                  const float* y, const int* lenR, long long strideR, int B, int up, int down,
                                  int half, const float* taps, const float* gains, const int* frames, int Tmax,
                                  float gain_const, float* out, hipStream_t stream) {
  if (!x || !u || !len16 || !y || !lenR || !out || !taps || B <= 0 || stride16 <= 0 || strideR <= 0) return SNRSE_EINVAL;
  if (up <= down || down <= 0 || gcd_ll(up, down) != 1 || half < 0 || half > (1 << 28)) return SNRSE_EINVAL;
  if (gains && (!frames || Tmax <= 0)) return SNRSE_EINVAL;
  const long long nblk = (strideR + HP - 1) / HP;
  if (nblk > 0x7fffffffLL) return SNRSE_EINVAL;
  const int K = (2 * half + up) / up;  // ceil((2 half + 1) / up)
  const long long span = ((long long)(HP - 1) * down) / up + K + 2;
  if (2 * span > HP_MAX_SPAN) return SNRSE_EINVAL;
  const dim3 grid((unsigned)nblk, (unsigned)(B < 65535 ? B : 65535));
  hipLaunchKernelGGL(resample_mix_kernel, grid, dim3(HP), (size_t)span * sizeof(float2), stream, x, u, len16,
                     stride16, y, lenR, strideR, B, up, down, half, K, taps, gains, frames, Tmax, gain_const, out);
  return (int)hipGetLastError();
}

extern "C" int snrse_band_gain(const float* u, const float* x, const int* lengths, int B, int Lstride, int Tmax,
                               double floor_gain, double* energies, float* gains, hipStream_t stream) {
  if (!u || !x || !lengths || !energies || !gains || B <= 0 || B > 65535 || Lstride <= 0 || Tmax <= 0)
    return SNRSE_EINVAL;
  if (!(floor_gain >= 0.0 && floor_gain <= 1.0)) return SNRSE_EINVAL;
  hipLaunchKernelGGL(band_energy_kernel, dim3((Tmax + FPB - 1) / FPB, B), dim3(256), 0, stream, u, x, lengths,
                     Lstride, Tmax, energies);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(band_gain_kernel, dim3((Tmax + 255) / 256, B), dim3(256), 0, stream, energies, lengths, B,
                     Lstride, Tmax, floor_gain, gains);
  return (int)hipGetLastError();
}
