// ESTOI, the extended short-time objective intelligibility measure (Jensen & Taal 2016, with pystoi's conventions;
// the definition is the comment of snrse_estoi in include/snrse.h), batched over a ragged [B][stride] pair of
// 10 kHz waveforms: x clean, y processed.  Five launches, whatever B is, no host synchronisation:
//
//   1 energy    one wave per frame of x: e_i = 20 log10(|w x_i|_2 + eps) in fp64 (window, products and sum)
//   2 compact   one workgroup per row: the row's maximum, the keep mask e_i > max - 40 and its stable compaction
//               (ballot prefix per wave, the wave totals through LDS, looped over the row's frames) -> the kept
//               frame indices f_0 < ... < f_{K-1} and K
//   3 spectrum  one workgroup per (row, EB re-framed frames); a wave takes one (frame, signal) at a time: the 256
//               samples of re-framed frame j are rebuilt from kept frames j - 1, j, j + 1 (the overlap-add signal
//               never reaches memory), windowed again, transformed by an in-place radix-2 decimation-in-frequency
//               FFT of 512 complex points in LDS (the input is real and half zeros; the results sit at bit-reversed
//               positions, which the band sums read directly) and reduced to the 15 third-octave band magnitudes
//               -> Xb, Yb [B][15][Mmax] f32
//   4 segment   one thread per segment m: its own 15 x 30 block of Xb and Yb, the row and the column normalisation
//               and the product sum in fp64 (two passes over the block, no running sums carried between segments);
//               a wave's 64 segments are folded by a shuffle butterfly -> partial [B][blocks]
//   5 finish    one thread per row adds the row's partials in ascending order -> out, info
//
// No floating-point atomics; every reduction has a fixed order that depends on the row alone, so a row's bits are
// the same on every launch, when the row is launched alone and wherever it stands in the batch.  Nothing at or
// past L_b of a row is read: every frame index is below nf_b = ceil((L_b - 256) / 128).
#include "common.h"

namespace {

constexpr int EF = 256;       // frame length
constexpr int EH = 128;       // hop
constexpr int ENFFT = 512;    // transform length
constexpr int ENB = 15;       // third-octave bands
constexpr int ESEG = 30;      // frames per segment
constexpr int EB = 8;         // re-framed frames per spectrum workgroup
constexpr int ET = 256;       // threads of the energy / compaction / spectrum workgroups
constexpr int ESB = 64;       // segments per segment workgroup (one wave)
constexpr double EEPS = 2.220446049250313e-16;
constexpr double EDYN = 40.0;
constexpr double ESENTINEL = 1e-5;

// bands [lo, hi) in bins of the 512-point spectrum at 10 kHz: centres 150 * 2^(k/3), edges the geometric means,
// snapped to the nearest bin
__constant__ int kBandLo[ENB + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

SNRSE_DEV int row_len(const int* lengths, int b, long long stride) {
  const long long L = lengths[b];
  return (int)(L < 0 ? 0 : (L > stride ? stride : L));
}
SNRSE_DEV int frames_of(int L) { return L > EF ? (L - EF + EH - 1) / EH : 0; }
// w[n] = 0.5 (1 - cos(2 pi (n + 1) / 257)), np.hanning(258)[1:-1]
SNRSE_DEV double hann(int n) { return 0.5 * (1.0 - cospi(2.0 * (double)(n + 1) / 257.0)); }

__global__ __launch_bounds__(ET) void estoi_energy_kernel(const float* __restrict__ x,
                                                          const int* __restrict__ lengths, int B, long long stride,
                                                          int nfa, double* __restrict__ E) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
  double w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = hann(lane + 64 * q);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int nf = frames_of(row_len(lengths, b, stride));
    if (i >= nf) continue;  // the same decision in every lane of the wave
    const float* xr = x + (size_t)b * (size_t)stride + (size_t)i * EH;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = w[q] * (double)xr[lane + 64 * q];
      s += v * v;
    }
    s = wave_sum_d(s);
    if (lane == 0) E[(size_t)b * nfa + i] = 20.0 * log10(sqrt(s) + EEPS);
  }
}

__global__ __launch_bounds__(ET) void estoi_compact_kernel(const int* __restrict__ lengths, int B, long long stride,
                                                           int nfa, const double* __restrict__ E,
                                                           int* __restrict__ idx, int* __restrict__ info) {
  __shared__ double red[ET / 64];
  __shared__ int cnt[ET / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int nf = frames_of(row_len(lengths, b, stride));
    const double* e = E + (size_t)b * nfa;
    int* id = idx + (size_t)b * nfa;
    double mx = -__builtin_inf();
    for (int i = tid; i < nf; i += ET) mx = fmax(mx, e[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    __syncthreads();  // the previous row's readers are done with red / cnt
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    const double thr = mx - EDYN;
    int base = 0;
    for (int i0 = 0; i0 < nf; i0 += ET) {  // uniform trip count
      const int i = i0 + tid;
      const bool keep = i < nf && e[i] > thr;
      const unsigned long long m = __ballot(keep);
      const int before = __popcll(m & ((1ull << lane) - 1ull));
      __syncthreads();
      if (lane == 0) cnt[wv] = __popcll(m);
      __syncthreads();
      int off = base;
      for (int q = 0; q < wv; ++q) off += cnt[q];
      if (keep) id[off + before] = i;
      base += cnt[0] + cnt[1] + cnt[2] + cnt[3];
    }
    if (tid == 0) info[2 * b] = base;
  }
}

__global__ __launch_bounds__(ET) void estoi_spectrum_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            int B, long long stride, int nfa, int Ma,
                                                            const int* __restrict__ idx,
                                                            const int* __restrict__ info, float* __restrict__ Xb,
                                                            float* __restrict__ Yb) {
  __shared__ float2 tw[ENFFT / 2];  // exp(-2 pi i q / 512)
  __shared__ float win[EF];
  __shared__ float2 zbuf[ET / 64][ENFFT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  {
    double sn, cs;
    sincospi(-(double)tid / 256.0, &sn, &cs);
    tw[tid] = make_float2((float)cs, (float)sn);
    win[tid] = (float)hann(tid);
  }
  float2* z = zbuf[wv];
  const int j0 = blockIdx.x * EB;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int K = info[2 * b], M = K - 1;
    if (j0 >= M) continue;  // the same decision in every thread
    const int* id = idx + (size_t)b * nfa;
    for (int t = wv; t < 2 * EB; t += ET / 64) {  // (frame, signal) tasks: 2 EB / 4 per wave, the same count in each
      const int j = j0 + (t >> 1);
      const bool live = j < M;
      const float* src = ((t & 1) ? y : x) + (size_t)b * (size_t)stride;
      __syncthreads();  // tables written; the previous task's readers are done with z
      if (live) {
        const int fc = id[j], fn = id[j + 1], fp = j > 0 ? id[j - 1] : -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = lane + 64 * q;
          float v = win[n] * src[(size_t)fc * EH + n];
          if (q < 2) {
            if (fp >= 0) v = fmaf(win[n + EH], src[(size_t)fp * EH + n + EH], v);
          } else {
            v = fmaf(win[n - EH], src[(size_t)fn * EH + n - EH], v);
          }
          z[n] = make_float2(v * win[n], 0.0f);
          z[n + EF] = make_float2(0.0f, 0.0f);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) z[lane + 64 * q] = make_float2(0.0f, 0.0f);
      }
      // decimation in frequency, in place: span h = 256 .. 1, butterfly r of group g: (a, b) -> (a + b, (a - b) W_2h^r)
      for (int h = ENFFT / 2, sh = 8; h >= 1; h >>= 1, --sh) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int u = lane + 64 * q;
          const int r = u & (h - 1);
          const int p = ((u >> sh) << (sh + 1)) + r;
          const float2 a = z[p], c = z[p + h];
          const float2 w = tw[r << (8 - sh)];
          const float dr = a.x - c.x, di = a.y - c.y;
          z[p] = make_float2(a.x + c.x, a.y + c.y);
          z[p + h] = make_float2(dr * w.x - di * w.y, dr * w.y + di * w.x);
        }
      }
      __syncthreads();
      // bin k of the spectrum sits at the bit-reversed position of k; a band has at most 45 bins: one per lane
      float mine = 0.0f;
#pragma unroll
      for (int k = 0; k < ENB; ++k) {
        const int bin = kBandLo[k] + lane;
        float s = 0.0f;
        if (bin < kBandLo[k + 1]) {
          const float2 v = z[__brev((unsigned)bin) >> 23];
          s = v.x * v.x + v.y * v.y;
        }
        s = wave_sum(s);
        if (lane == k) mine = sqrtf(s);
      }
      if (live && lane < ENB) ((t & 1) ? Yb : Xb)[((size_t)b * ENB + lane) * (size_t)Ma + j] = mine;
    }
  }
}

__global__ __launch_bounds__(ESB) void estoi_segment_kernel(int B, int Ma, int nsb, const int* __restrict__ info,
                                                            const float* __restrict__ Xb,
                                                            const float* __restrict__ Yb,
                                                            double* __restrict__ partial) {
  const int m = blockIdx.x * ESB + threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int S = info[2 * b] - 1 - (ESEG - 1);
    if (blockIdx.x * ESB >= S) continue;  // the same decision in every lane
    double d = 0.0;
    if (m < S) {
      const float* px = Xb + (size_t)b * ENB * (size_t)Ma + m;
      const float* py = Yb + (size_t)b * ENB * (size_t)Ma + m;
      // rows: mean over the 30 frames and the L2 norm of the centred row
      double mxr[ENB], myr[ENB], nxr[ENB], nyr[ENB];
#pragma unroll
      for (int k = 0; k < ENB; ++k) {
        double sx = 0.0, sy = 0.0;
        for (int j = 0; j < ESEG; ++j) {
          sx += (double)px[(size_t)k * Ma + j];
          sy += (double)py[(size_t)k * Ma + j];
        }
        sx /= ESEG;
        sy /= ESEG;
        double qx = 0.0, qy = 0.0;
        for (int j = 0; j < ESEG; ++j) {
          const double vx = (double)px[(size_t)k * Ma + j] - sx, vy = (double)py[(size_t)k * Ma + j] - sy;
          qx += vx * vx;
          qy += vy * vy;
        }
        mxr[k] = sx;
        myr[k] = sy;
        nxr[k] = sqrt(qx) + EEPS;
        nyr[k] = sqrt(qy) + EEPS;
      }
      // columns: the row-normalised values of frame j, centred over the 15 bands and divided by their norm
      for (int j = 0; j < ESEG; ++j) {
        double ax[ENB], ay[ENB], sx = 0.0, sy = 0.0;
#pragma unroll
        for (int k = 0; k < ENB; ++k) {
          ax[k] = ((double)px[(size_t)k * Ma + j] - mxr[k]) / nxr[k];
          ay[k] = ((double)py[(size_t)k * Ma + j] - myr[k]) / nyr[k];
          sx += ax[k];
          sy += ay[k];
        }
        sx /= ENB;
        sy /= ENB;
        double qx = 0.0, qy = 0.0;
#pragma unroll
        for (int k = 0; k < ENB; ++k) {
          ax[k] -= sx;
          ay[k] -= sy;
          qx += ax[k] * ax[k];
          qy += ay[k] * ay[k];
        }
        const double ix = sqrt(qx) + EEPS, iy = sqrt(qy) + EEPS;
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < ENB; ++k) c += (ax[k] / ix) * (ay[k] / iy);
        d += c;
      }
    }
    d = wave_sum_d(d);
    if (threadIdx.x == 0) partial[(size_t)b * nsb + blockIdx.x] = d;
  }
}

__global__ __launch_bounds__(64) void estoi_finish_kernel(int B, int nsb, const double* __restrict__ partial,
                                                          double* __restrict__ out, int* __restrict__ info) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int S = info[2 * b] - 1 - (ESEG - 1);
  if (S <= 0) {
    out[b] = ESENTINEL;
    info[2 * b + 1] = 0;
    return;
  }
  double d = 0.0;
  for (int q = 0; q < (S + ESB - 1) / ESB; ++q) d += partial[(size_t)b * nsb + q];
  out[b] = d / ((double)ESEG * (double)S);
  info[2 * b + 1] = S;
}

struct Plan {
  int nfa, Ma, nsb;
  size_t offE, offIdx, offX, offY, offP, bytes;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

Plan plan_of(int B, long long stride) {
  Plan p;
  const long long Lmax = stride > 0x7fffffffLL ? 0x7fffffffLL : stride;  // the lengths are int32
  const long long nf = Lmax > EF ? (Lmax - EF + EH - 1) / EH : 0;
  p.nfa = (int)(nf > 1 ? nf : 1);
  p.Ma = (int)(nf > 2 ? nf - 1 : 1);
  const int smax = p.Ma > ESEG ? p.Ma - (ESEG - 1) : 1;
  p.nsb = (smax + ESB - 1) / ESB;
  size_t o = 0;
  p.offE = o;
  o = align256(o + (size_t)B * p.nfa * sizeof(double));
  p.offIdx = o;
  o = align256(o + (size_t)B * p.nfa * sizeof(int));
  p.offX = o;
  o = align256(o + (size_t)B * ENB * p.Ma * sizeof(float));
  p.offY = o;
  o = align256(o + (size_t)B * ENB * p.Ma * sizeof(float));
  p.offP = o;
  o = align256(o + (size_t)B * p.nsb * sizeof(double));
  p.bytes = o;
  return p;
}

}  // namespace

extern "C" int snrse_estoi_block(void) { return EB; }

extern "C" size_t snrse_estoi_workspace(int B, long long stride) {
  if (B <= 0 || stride <= 0) return 0;
  return plan_of(B, stride).bytes;
}

extern "C" int snrse_estoi(const float* x, const float* y, const int* lengths, int B, long long stride, void* work,
                           size_t work_bytes, double* out, int* info, hipStream_t stream) {
  if (B <= 0 || stride <= 0 || !x || !y || !lengths || !work || !out || !info) return SNRSE_EINVAL;
  const Plan p = plan_of(B, stride);
  if (work_bytes < p.bytes) return SNRSE_EINVAL;
  char* ws = (char*)work;
  double* E = (double*)(ws + p.offE);
  int* idx = (int*)(ws + p.offIdx);
  float* Xb = (float*)(ws + p.offX);
  float* Yb = (float*)(ws + p.offY);
  double* partial = (double*)(ws + p.offP);
  const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
  hipLaunchKernelGGL(estoi_energy_kernel, dim3((unsigned)((p.nfa + ET / 64 - 1) / (ET / 64)), gy), dim3(ET), 0,
                     stream, x, lengths, B, stride, p.nfa, E);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(estoi_compact_kernel, dim3(gy), dim3(ET), 0, stream, lengths, B, stride, p.nfa, E, idx, info);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(estoi_spectrum_kernel, dim3((unsigned)((p.Ma + EB - 1) / EB), gy), dim3(ET), 0, stream, x, y, B,
                     stride, p.nfa, p.Ma, idx, info, Xb, Yb);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(estoi_segment_kernel, dim3((unsigned)p.nsb, gy), dim3(ESB), 0, stream, B, p.Ma, p.nsb, info, Xb,
                     Yb, partial);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(estoi_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, B, p.nsb, partial,
                     out, info);
  return (int)hipGetLastError();
}
