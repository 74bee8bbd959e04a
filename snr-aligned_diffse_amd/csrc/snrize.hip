// Fixed-SNR dataset preparation (snrse.snrize): the active-level analysis of a clean / noise pair and its remix to
// a target active SNR, over a ragged batch [B][stride] f32 with lengths [B].
//
//   snrse_active_window_sums   per 100-ms window sum c^2, sum n^2 (f64); per row max |n|; per block the five
//                              sums of the Pearson coefficient
//   snrse_active_finalize      activity mask (decided by the noise), active RMS of both, Pearson, gain g
//   snrse_snr_mix              n' = g n, y = c + n', per row max |y|
//   snrse_scale_to_pcm16       clip guard s from max |y| on the device, the three signals scaled and as int16
//
// All four stream their rows once (HBM-bound: the analysis reads 8 B per sample, the mix reads 8 B and writes 8 B,
// the PCM pass reads 12 B and writes 6 B, plus 12 B when the scaled floats are wanted); the work is in the order
// of the sums.  No f64 atomics: a window is summed by one wave, lane l taking the window's samples
// [4 (l + 64 j), 4 (l + 64 j) + 4) for j = 0, 1, .. in that order -- indices relative to the WINDOW, not to a 16-B
// boundary, so the order does not change with the row's address -- followed by a butterfly over the lanes; the
// windows are folded in ascending order by the finalize kernel, and so are the blocks' partial sums.  A row's
// numbers therefore do not depend on its position in the batch, on the rows it shares the launch with, or on how
// its buffer is aligned.  The only atomics are integer maxima of |v| bit patterns (csrc/range.hip), which commute.
//
// Loads are 16 B wide over the part of a window that lies 16-B vectors inside its row: one vector where the
// window's groups of four are aligned, else the two aligned vectors a group straddles (the second is the next
// lane's first: an L1 hit, no extra HBM traffic); scalar loads for the groups at a row's or window's edge.
// Compiled without fp contraction (snrse/build.py): the remix is exactly the expressions written in snr_mix_kernel.
#include "common.h"

namespace {

constexpr int AT = 256;           // threads per block of every kernel here
constexpr int AWAVES = AT / 64;   // waves per block
constexpr int WPB = 8;            // windows a block of the analysis owns (two per wave)
constexpr double kEps = 2.220446049250313e-16;  // numpy's float64 eps, as the definition uses it

SNRSE_DEV uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

SNRSE_DEV int row_length(const int* lengths, int b, long long stride) {
  const long long L = lengths[b];
  return (int)(L < 0 ? 0 : (L > stride ? stride : L));
}

// samples [i0, i0 + 4) of `row`, zero from `we` (the window's end) on; mis = elements (row + i0) lies past a 16-B
// boundary; nothing outside [0, L) is read
SNRSE_DEV void load4(const float* __restrict__ row, long long i0, int mis, long long we, long long L, float (&v)[4]) {
  if (i0 + 4 <= we) {
    if (mis == 0) {
      const f32x4 t = *(const f32x4*)(row + i0);
      v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
      return;
    }
    const long long a = i0 - mis;
    if (a >= 0 && a + 8 <= L) {
      const f32x4 lo = *(const f32x4*)(row + a), hi = *(const f32x4*)(row + a + 4);
      if (mis == 1) {
        v[0] = lo[1], v[1] = lo[2], v[2] = lo[3], v[3] = hi[0];
      } else if (mis == 2) {
        v[0] = lo[2], v[1] = lo[3], v[2] = hi[0], v[3] = hi[1];
      } else {
        v[0] = lo[3], v[1] = hi[0], v[2] = hi[1], v[3] = hi[2];
      }
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = i0 + k < we ? row[i0 + k] : 0.0f;
}

// grid (chunks of WPB windows, rows).  wsums [B][nWmax][2] = (sum c^2, sum n^2) of each window of each row (windows
// past a row's last are not written); partials [B][nchunks][5] = (sum c, sum n, sum c^2, sum n^2, sum c n) of the
// block's windows; nmax [B] zeroed by the caller, max |n| as a bit pattern.
__global__ __launch_bounds__(AT) void active_window_sums_kernel(const float* __restrict__ c,
                                                                const float* __restrict__ n,
                                                                const int* __restrict__ lengths, int B,
                                                                long long stride, int W, int nWmax, int nchunks,
                                                                double* __restrict__ wsums,
                                                                double* __restrict__ partials,
                                                                unsigned int* __restrict__ nmax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ double s_red[AWAVES][5];
  __shared__ uint32_t s_pk[AWAVES];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const long long nW = (L + W - 1) / W;
    const long long k0 = (long long)blockIdx.x * WPB;
    if (k0 >= nW) continue;  // uniform over the block
    const float* pc = c + (size_t)b * (size_t)stride;
    const float* pn = n + (size_t)b * (size_t)stride;
    const long long k1 = k0 + WPB < nW ? k0 + WPB : nW;
    double sc = 0, sn = 0, scn = 0;  // per lane, over the wave's windows
    double tcc = 0, tnn = 0;         // the wave's windows, each already reduced
    uint32_t pk = 0;
    for (long long k = k0 + wave; k < k1; k += AWAVES) {
      const long long ws = k * W;
      const long long we = ws + W < L ? ws + W : L;
      const int ng = (int)((we - ws + 3) >> 2);
      const int mc = (int)(((uintptr_t)(pc + ws) >> 2) & 3), mn = (int)(((uintptr_t)(pn + ws) >> 2) & 3);
      double cc = 0, nn = 0;
      for (int g = lane; g < ng; g += 64) {
        const long long i0 = ws + 4LL * g;
        float vc[4], vn[4];
        load4(pc, i0, mc, we, L, vc);
        load4(pn, i0, mn, we, L, vn);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double x = vc[j], z = vn[j];  // every product of two f32 is exact in f64
          cc += x * x;
          nn += z * z;
          sc += x;
          sn += z;
          scn += x * z;
          pk = max(pk, abs_bits(vn[j]));
        }
      }
      cc = wave_sum_d(cc);
      nn = wave_sum_d(nn);
      if (lane == 0) {
        double* o = wsums + ((size_t)b * (size_t)nWmax + (size_t)k) * 2;
        o[0] = cc;
        o[1] = nn;
      }
      tcc += cc;
      tnn += nn;
    }
    sc = wave_sum_d(sc);
    sn = wave_sum_d(sn);
    scn = wave_sum_d(scn);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = max(pk, (uint32_t)__shfl_xor((int)pk, o, 64));
    if (lane == 0) {
      s_red[wave][0] = sc, s_red[wave][1] = sn, s_red[wave][2] = tcc, s_red[wave][3] = tnn, s_red[wave][4] = scn;
      s_pk[wave] = pk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double* o = partials + ((size_t)b * (size_t)nchunks + blockIdx.x) * 5;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        double d = s_red[0][j];
#pragma unroll
        for (int w = 1; w < AWAVES; ++w) d += s_red[w][j];
        o[j] = d;
      }
#pragma unroll
      for (int w = 1; w < AWAVES; ++w) pk = max(pk, s_pk[w]);
      if (pk) atomicMax(nmax + b, pk);
    }
    __syncthreads();  // s_red / s_pk are reused by the next row of this block
  }
}

// One wave per row.  out [B][5] = clean_rms, noise_rms, active windows, Pearson coefficient, gain.
__global__ __launch_bounds__(64) void active_finalize_kernel(const double* __restrict__ wsums,
                                                             const double* __restrict__ partials,
                                                             const float* __restrict__ nmax,
                                                             const int* __restrict__ lengths, int B, long long stride,
                                                             int W, int nWmax, int nchunks, double thr,
                                                             const double* __restrict__ snr_db,
                                                             double* __restrict__ out) {
  const int lane = threadIdx.x;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const long long L = row_length(lengths, b, stride);
    const long long nW = (L + W - 1) / W;
    // window k is active iff sqrt(mean n_k^2) > thr (max |n| + eps), in f64 as written
    const double limit = thr * ((double)nmax[b] + kEps);
    const double* ws = wsums + (size_t)b * (size_t)nWmax * 2;
    double ac = 0, an = 0;
    long long acnt = 0, nact = 0;
    for (long long kb = 0; kb < nW; kb += 64) {
      const long long k = kb + lane;
      double vc = 0, vn = 0;
      long long cnt = 0;
      if (k < nW) {
        const long long left = L - k * W;
        const long long m = left < W ? left : W;
        const double cc = ws[2 * k], nn = ws[2 * k + 1];
        if (sqrt(nn / (double)m) > limit) vc = cc, vn = nn, cnt = m;
      }
      // ascending window order, every lane the same sum; an inactive window adds +0, which changes nothing
      const int m64 = (int)(nW - kb < 64 ? nW - kb : 64);
      for (int l = 0; l < m64; ++l) {
        ac += __shfl(vc, l, 64);
        an += __shfl(vn, l, 64);
      }
      nact += __popcll(__ballot(cnt > 0));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      acnt += cnt;
    }
    // the blocks' partial sums in ascending order
    const long long nch = (nW + WPB - 1) / WPB;
    double s[5] = {0, 0, 0, 0, 0};
    for (long long j = 0; j < nch; ++j) {
      const double* p = partials + ((size_t)b * (size_t)nchunks + (size_t)j) * 5;
#pragma unroll
      for (int q = 0; q < 5; ++q) s[q] += p[q];
    }
    if (lane != 0) continue;
    double crms = kEps, nrms = kEps;
    if (acnt > 0) {
      crms = sqrt(ac / (double)acnt);
      nrms = sqrt(an / (double)acnt);
    }
    const double N = (double)L;
    const double vcc = N * s[2] - s[0] * s[0], vnn = N * s[3] - s[1] * s[1];
    const double den = sqrt(vcc) * sqrt(vnn);
    const double corr = (vcc > 0 && vnn > 0 && den > 0) ? (N * s[4] - s[0] * s[1]) / den : 0.0;
    double* o = out + (size_t)b * 5;
    o[0] = crms;
    o[1] = nrms;
    o[2] = (double)nact;
    o[3] = corr;
    o[4] = (crms / nrms) * pow(10.0, -snr_db[b] / 20.0);
  }
}

// The split of a row for the two elementwise kernels: when every row pointer sits the same `mis` elements past a
// 16-B boundary, [head, head + 4 nvec) is 16-B aligned in all of them and goes by vectors; the rest (fewer than 8
// elements, or the whole row when the pointers disagree) goes by scalars.
struct RowSplit {
  long long head, nvec, tail0, nscalar;
};
SNRSE_DEV RowSplit split_row(int mis, long long stride) {
  RowSplit r;
  if (mis < 0) {
    r.head = stride, r.nvec = 0, r.tail0 = stride, r.nscalar = stride;
    return r;
  }
  r.head = mis ? 4 - mis : 0;
  if (r.head > stride) r.head = stride;
  r.nvec = (stride - r.head) / 4;
  r.tail0 = r.head + r.nvec * 4;
  r.nscalar = r.head + (stride - r.tail0);
  return r;
}
// the common misalignment (in elements) of float pointers, -1 when they differ; NULL pointers do not count
SNRSE_DEV int common_mis(const float* const* p, int np) {
  int mis = -2;
  for (int i = 0; i < np; ++i) {
    if (!p[i]) continue;
    const int m = (int)(((uintptr_t)p[i] >> 2) & 3);
    if (mis == -2) mis = m;
    else if (mis != m) return -1;
  }
  return mis < 0 ? -1 : mis;
}

SNRSE_DEV uint32_t block_max_bits(uint32_t pk, uint32_t* s_pk) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pk = max(pk, (uint32_t)__shfl_xor((int)pk, o, 64));
  if ((threadIdx.x & 63) == 0) s_pk[threadIdx.x >> 6] = pk;
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int w = 1; w < AWAVES; ++w) pk = max(pk, s_pk[w]);
  return pk;  // thread 0's value is the block's
}

// n' = gf n and y = fma(gf, n, c) with gf = (float)g: n' carries two roundings (g to f32, the product), y two
// (g to f32, the fma's one) -- y is NOT c + n' rounded again.  Elements from L_b to the stride are written as 0.
__global__ __launch_bounds__(AT) void snr_mix_kernel(const float* __restrict__ c, const float* __restrict__ n,
                                                     const int* __restrict__ lengths, int B, long long stride,
                                                     const double* __restrict__ gain, int gain_stride,
                                                     float* __restrict__ n_out, float* __restrict__ y_out,
                                                     unsigned int* __restrict__ ymax) {
  __shared__ uint32_t s_pk[AWAVES];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const size_t off = (size_t)b * (size_t)stride;
    const float *pc = c + off, *pn = n + off;
    float *po = n_out + off, *py = y_out + off;
    const float gf = (float)gain[(size_t)b * (size_t)gain_stride];
    const float* ptrs[4] = {pc, pn, po, py};
    const RowSplit sp = split_row(common_mis(ptrs, 4), stride);
    uint32_t pk = 0;
    for (long long v = (long long)blockIdx.x * AT + threadIdx.x; v < sp.nvec; v += (long long)gridDim.x * AT) {
      const long long i = sp.head + 4 * v;
      f32x4 o = {0.f, 0.f, 0.f, 0.f}, y = {0.f, 0.f, 0.f, 0.f};
      if (i < L) {
        const f32x4 vc = *(const f32x4*)(pc + i), vn = *(const f32x4*)(pn + i);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i + j < L) {
            o[j] = gf * vn[j];
            y[j] = fmaf(gf, vn[j], vc[j]);
            pk = max(pk, abs_bits(y[j]));
          }
      }
      *(f32x4*)(po + i) = o;
      *(f32x4*)(py + i) = y;
    }
    for (long long q = (long long)blockIdx.x * AT + threadIdx.x; q < sp.nscalar; q += (long long)gridDim.x * AT) {
      const long long i = q < sp.head ? q : sp.tail0 + (q - sp.head);
      float o = 0.f, y = 0.f;
      if (i < L) {
        const float vn = pn[i];
        o = gf * vn;
        y = fmaf(gf, vn, pc[i]);
        pk = max(pk, abs_bits(y));
      }
      po[i] = o;
      py[i] = y;
    }
    pk = block_max_bits(pk, s_pk);
    if (threadIdx.x == 0 && pk) atomicMax(ymax + b, pk);
    __syncthreads();
  }
}

// v -> int16 as numpy's clip(round(v * 32768), -32768, 32767): the product is exact (a power of two), rintf rounds
// half to even, the clamp saturates; a NaN becomes 0
SNRSE_DEV short to_pcm16(float v) {
  const float r = rintf(v * 32768.0f);
  return (short)(int)fminf(fmaxf(r, -32768.0f), 32767.0f);
}

// s_b = max |y| > 0.99 ? (0.99 - eps) / max |y| : 1 in f64 from the mix kernel's row maximum, applied as one f32
// product x * (float)s_b (s_b = 1: the values pass unchanged).  Float outputs may alias their inputs; each output
// pointer may be NULL.  Blocks with blockIdx.x == 0 also write scale[b].
__global__ __launch_bounds__(AT) void scale_to_pcm16_kernel(const float* c, const float* n1, const float* y,
                                                            const int* __restrict__ lengths, int B, long long stride,
                                                            const float* __restrict__ ymax, float* c_f, float* n_f,
                                                            float* y_f, short* __restrict__ c_q,
                                                            short* __restrict__ n_q, short* __restrict__ y_q,
                                                            double* __restrict__ scale) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long L = row_length(lengths, b, stride);
    const size_t off = (size_t)b * (size_t)stride;
    const double pkd = (double)ymax[b];
    const double s = pkd > 0.99 ? (0.99 - kEps) / pkd : 1.0;
    const float sf = (float)s;
    if (blockIdx.x == 0 && threadIdx.x == 0) scale[b] = s;
    const float* in[3] = {c + off, n1 + off, y + off};
    float* of[3] = {c_f ? c_f + off : nullptr, n_f ? n_f + off : nullptr, y_f ? y_f + off : nullptr};
    short* oq[3] = {c_q ? c_q + off : nullptr, n_q ? n_q + off : nullptr, y_q ? y_q + off : nullptr};
    const float* ptrs[6] = {in[0], in[1], in[2], of[0], of[1], of[2]};
    const RowSplit sp = split_row(common_mis(ptrs, 6), stride);
    for (long long v = (long long)blockIdx.x * AT + threadIdx.x; v < sp.nvec; v += (long long)gridDim.x * AT) {
      const long long i = sp.head + 4 * v;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (i < L) {
          const f32x4 r = *(const f32x4*)(in[t] + i);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j < L) x[j] = r[j] * sf;
        }
        if (of[t]) *(f32x4*)(of[t] + i) = x;
        if (oq[t]) {
          short* q = oq[t] + i;
          const short q0 = to_pcm16(x[0]), q1 = to_pcm16(x[1]), q2 = to_pcm16(x[2]), q3 = to_pcm16(x[3]);
          if (((uintptr_t)q & 7) == 0) {
            uint2 w;
            w.x = (uint32_t)(uint16_t)q0 | ((uint32_t)(uint16_t)q1 << 16);
            w.y = (uint32_t)(uint16_t)q2 | ((uint32_t)(uint16_t)q3 << 16);
            *(uint2*)q = w;
          } else {
            q[0] = q0, q[1] = q1, q[2] = q2, q[3] = q3;
          }
        }
      }
    }
    for (long long p = (long long)blockIdx.x * AT + threadIdx.x; p < sp.nscalar; p += (long long)gridDim.x * AT) {
      const long long i = p < sp.head ? p : sp.tail0 + (p - sp.head);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const float x = i < L ? in[t][i] * sf : 0.0f;
        if (of[t]) of[t][i] = x;
        if (oq[t]) oq[t][i] = to_pcm16(x);
      }
    }
  }
}

// blocks per row of the elementwise kernels: four 16-B vectors per thread, at most ~2048 blocks in the launch
unsigned blocks_per_row(long long stride, int rows) {
  long long bpr = (stride / 4 + (long long)AT * 4 - 1) / ((long long)AT * 4);
  const long long cap = 2048 / rows > 1 ? 2048 / rows : 1;
  bpr = bpr < 1 ? 1 : (bpr > cap ? cap : bpr);
  return (unsigned)bpr;
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" int snrse_active_windows_per_block(void) { return WPB; }

extern "C" int snrse_active_window_sums(const float* c, const float* n, const int* lengths, int B, long long stride,
                                        int W, double* wsums, double* partials, float* nmax, hipStream_t stream) {
  if (!c || !n || !lengths || !wsums || !partials || !nmax || B <= 0 || stride <= 0 || W <= 0) return SNRSE_EINVAL;
  if (stride > 0x7fffffffLL || !aligned4(c) || !aligned4(n)) return SNRSE_EINVAL;
  const long long nWmax = (stride + W - 1) / W;
  const long long nchunks = (nWmax + WPB - 1) / WPB;
  SNRSE_RET(hipMemsetAsync(nmax, 0, (size_t)B * sizeof(float), stream));
  const dim3 grid((unsigned)nchunks, (unsigned)(B < 65535 ? B : 65535));
  hipLaunchKernelGGL(active_window_sums_kernel, grid, dim3(AT), 0, stream, c, n, lengths, B, stride, W, (int)nWmax,
                     (int)nchunks, wsums, partials, (unsigned int*)nmax);
  return (int)hipGetLastError();
}

extern "C" int snrse_active_finalize(const double* wsums, const double* partials, const float* nmax,
                                     const int* lengths, int B, long long stride, int W, const double* snr_db,
                                     double* out, hipStream_t stream) {
  if (!wsums || !partials || !nmax || !lengths || !snr_db || !out || B <= 0 || stride <= 0 || W <= 0)
    return SNRSE_EINVAL;
  if (stride > 0x7fffffffLL) return SNRSE_EINVAL;
  const long long nWmax = (stride + W - 1) / W;
  const long long nchunks = (nWmax + WPB - 1) / WPB;
  const double thr = pow(10.0, -50.0 / 20.0);
  hipLaunchKernelGGL(active_finalize_kernel, dim3((unsigned)(B < 1048576 ? B : 1048576)), dim3(64), 0, stream, wsums,
                     partials, nmax, lengths, B, stride, W, (int)nWmax, (int)nchunks, thr, snr_db, out);
  return (int)hipGetLastError();
}

extern "C" int snrse_snr_mix(const float* c, const float* n, const int* lengths, int B, long long stride,
                             const double* gain, int gain_stride, float* n_out, float* y_out, float* ymax,
                             hipStream_t stream) {
  if (!c || !n || !lengths || !gain || !n_out || !y_out || !ymax || B <= 0 || stride <= 0 || gain_stride <= 0)
    return SNRSE_EINVAL;
  if (stride > 0x7fffffffLL || !aligned4(c) || !aligned4(n) || !aligned4(n_out) || !aligned4(y_out))
    return SNRSE_EINVAL;
  SNRSE_RET(hipMemsetAsync(ymax, 0, (size_t)B * sizeof(float), stream));
  const int rows = B < 65535 ? B : 65535;
  hipLaunchKernelGGL(snr_mix_kernel, dim3(blocks_per_row(stride, rows), (unsigned)rows), dim3(AT), 0, stream, c, n,
                     lengths, B, stride, gain, gain_stride, n_out, y_out, (unsigned int*)ymax);
  return (int)hipGetLastError();
}

extern "C" int snrse_scale_to_pcm16(const float* c, const float* n1, const float* y, const int* lengths, int B,
                                    long long stride, const float* ymax, float* c_f, float* n_f, float* y_f,
                                    short* c_q, short* n_q, short* y_q, double* scale, hipStream_t stream) {
  if (!c || !n1 || !y || !lengths || !ymax || !scale || B <= 0 || stride <= 0) return SNRSE_EINVAL;
  if (stride > 0x7fffffffLL) return SNRSE_EINVAL;
  const void* f[6] = {c, n1, y, c_f, n_f, y_f};
  for (const void* p : f)
    if (!aligned4(p)) return SNRSE_EINVAL;
  const void* q[3] = {c_q, n_q, y_q};
  for (const void* p : q)
    if ((uintptr_t)p & 1) return SNRSE_EINVAL;
  const int rows = B < 65535 ? B : 65535;
  hipLaunchKernelGGL(scale_to_pcm16_kernel, dim3(blocks_per_row(stride, rows), (unsigned)rows), dim3(AT), 0, stream,
                     c, n1, y, lengths, B, stride, ymax, c_f, n_f, y_f, c_q, n_q, y_q, scale);
  return (int)hipGetLastError();
}
