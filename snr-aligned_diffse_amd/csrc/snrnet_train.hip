// Training of the SNR estimator (reference sgmse/snr_estimator.py:81-116 around SNRNet, snrnet.py:47-97)
// on gfx950, fp32: the batch perturbation, a forward that saves what the backward needs, and the backward.
//
//   snrse_snr_perturb        y' = (x + (y - x) 0.56234 SNR) 2.040166 / sqrt(1 + SNR^2), SNR = gt / (1 - gt)
//   snrse_snrnet_train_fwd   the stage kernels of snrnet_stages.h with SAVE = true (same arithmetic as
//                            snrse_snrnet) + pool winners (u8), LSTM gate activations / cell states, head
//                            argmin / argmax; the pre-pool conv outputs are never stored
//   snrse_snrnet_backward    d est [B] -> the 17 packed gradient tensors (layout of ops.pack_snrnet):
//     head         (mean, std, min, max over S; FC; sigmoid)          -> dh [B,S,256], dfc
//     BiLSTM BPTT  one workgroup per (b, dir), W_hh by columns in registers, Whh^T dgates through LDS
//                  -> dgates [2][B S][512], h_prev [2][B S][128]; dW_hh, dW_ih, dfeat on snrse_bgemm
//     time convs   dfeat routed to the winning position: dW_k (a gather per (n, co), every thread owns
//                  its destinations and walks the chunks: no atomics), da2
//     conv3x3      da2 routed to the pool winner: dgrad (the forward's tiling with flipped weights) -> da1,
//                  wgrad over the pooled positions only (the other conv rows have zero gradient)
//     conv5x5      da1 routed to the 2x2 winner: wgrad, reading the spectrogram in place
// Weight-gradient reductions over N x pixels: registers over a workgroup's work units, one partial slab
// per workgroup, a sum pass over the slabs.  No atomics anywhere: the backward is run-to-run reproducible.
#include "snrnet_stages.h"

extern "C" int snrse_bgemm(const float* A, long long sAb, long long sAm, long long sAk, const float* Bm,
                           long long sBb, long long sBk, long long sBn, float* C, long long sCb, long long sCm,
                           long long sCn, const float* bias, int batch, int M, int N, int K, float alpha, float beta,
                           hipStream_t s);

namespace {

constexpr int WG_SLABS = 256;             // workgroups (= partial slabs) of the conv weight-gradient kernels
constexpr int SLAB = 32 * 32 * 9 + 32;    // floats per slab: dW3 + db3 (dW5 + db5 = 1632 fits)

// Byte offsets into the training workspace (every region 256-B aligned).
struct Layout {
  size_t a1, a2, feat, xg, hout, gates, cst, arg, win1, win2, winp;          // saved by the forward
  size_t dh, dgates, hprev, dfeat, da2, da1, stats, dz, slabs;               // backward scratch
  size_t bytes;
};
Layout layout(int B, int T) {
  const size_t S = T / 16, N = (size_t)B * S;
  Layout L{};
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 255) & ~(size_t)255; return at; };
  L.a1 = take(4 * N * 32 * 128 * 8);
  L.a2 = take(4 * N * 32 * 64 * 8);
  L.feat = take(4 * N * 128);
  L.xg = take(4 * N * 2 * 512);
  L.hout = take(4 * N * 256);
  L.gates = take(4 * N * 2 * 512);
  L.cst = take(4 * N * 2 * 128);
  L.arg = take(4 * (size_t)B * 512);
  L.win1 = take(N * 32 * 128 * 8);
  L.win2 = take(N * 32 * 64 * 8);
  L.winp = take(N * 128);
  L.dh = take(4 * N * 256);
  L.dgates = take(4 * N * 2 * 512);
  L.hprev = take(4 * N * 2 * 128);
  L.dfeat = take(4 * N * 128);
  L.da2 = take(4 * N * 32 * 64 * 8);
  L.da1 = take(4 * N * 32 * 128 * 8);
  L.stats = take(4 * (size_t)B * 1024);
  L.dz = take(4 * (size_t)B);
  L.slabs = take(4 * (size_t)WG_SLABS * SLAB);
  L.bytes = o;
  return L;
}

// ------------------------------------------------------------------------------------------ perturbation
// snr_estimator.py:93-98 on interleaved complex64 [B][per]; normfac = calculate_normfac_direct(1, SNR, 1)
__global__ __launch_bounds__(256) void snr_perturb_kernel(const float2* x, const float2* y, const float* gt,
                                                          long long per, long long n, float2* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float g = gt[i / per];
  const float snr = g / (1.f - g);
  const float nf = 2.040166f / sqrtf(1.f + snr * snr);  // (0.240253 + 0.759747 * 1^2)^0.5 = 1
  const float2 xv = x[i], yv = y[i];
  out[i] = make_float2((xv.x + (yv.x - xv.x) * 0.56234f * snr) * nf, (xv.y + (yv.y - xv.y) * 0.56234f * snr) * nf);
}

// ------------------------------------------------------------------------------------------ head backward
// block b, thread j: the statistics of h[b, :, j] as the forward computes them (stats [B][4][256] for the FC
// weight gradient), dz = d est * est (1 - est), and dh[b, s, j] through mean / unbiased std / min / max.
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* hout, const int* arg, const float* fcw,
                                                       const float* est, const float* dest, int S, float* dh,
                                                       float* stats, float* dz) {
  const int b = blockIdx.x, j = threadIdx.x;
  const float* hb = hout + (size_t)b * S * 256;
  double s1 = 0.0;
  for (int s = 0; s < S; ++s) s1 += hb[s * 256 + j];
  const double mean = s1 / S;
  double s2 = 0.0;
  for (int s = 0; s < S; ++s) {
    const double d = hb[s * 256 + j] - mean;
    s2 += d * d;
  }
  const float sd = (float)sqrt(s2 / (S - 1));
  const int amn = arg[b * 512 + j], amx = arg[b * 512 + 256 + j];
  float* st = stats + (size_t)b * 1024;
  st[j] = (float)mean;
  st[256 + j] = sd;
  st[512 + j] = hb[amn * 256 + j];
  st[768 + j] = hb[amx * 256 + j];
  const float e = est[b];
  const float z = dest[b] * e * (1.f - e);
  if (j == 0) dz[b] = z;
  const float gm = fcw[j] * z / (float)S;
  const float gs = fcw[256 + j] * z / ((float)(S - 1) * sd);  // sd = 0: NaN, as torch's std backward
  const float gn = fcw[512 + j] * z, gx = fcw[768 + j] * z;
  float* d = dh + (size_t)b * S * 256;
  for (int s = 0; s < S; ++s) {
    float v = gm + gs * (hb[s * 256 + j] - (float)mean);
    if (s == amn) v += gn;
    if (s == amx) v += gx;
    d[s * 256 + j] = v;
  }
}

__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* stats, const float* dz, int B, float* dfcw,
                                                         float* dfcb) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // 0 .. 1023
  float acc = 0.f, zb = 0.f;
  for (int b = 0; b < B; ++b) {
    acc = fmaf(dz[b], stats[(size_t)b * 1024 + i], acc);
    zb += dz[b];
  }
  dfcw[i] = acc;
  if (i == 0) dfcb[0] = zb;
}

// ------------------------------------------------------------------------------------------ LSTM BPTT
// block (b, dir), 512 threads, the steps in reverse of lstm_rec_kernel's order.  Threads g < 128 own hidden unit
// g: they turn dh + the carried hidden gradient into the four pre-activation gate gradients (LDS + global).
// Then all 512 threads form Whh^T dgates: thread (q, k) holds column k of the gate rows [128 q, 128 q + 128)
// in registers for all S steps and writes its partial dot to LDS; the owners sum the four partials.
__global__ __launch_bounds__(512) void lstm_bwd_kernel(const float* dh, const float* gates, const float* cst,
                                                       const float* hout, const float* whh, int B, int S,
                                                       float* dgates, float* hprev) {
  __shared__ __attribute__((aligned(16))) float dgl[512];
  __shared__ float part[4][128];
  const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, t = threadIdx.x;
  const int k = t & 127, q = __builtin_amdgcn_readfirstlane(t >> 7);
  float wc[128];
#pragma unroll
  for (int i = 0; i < 128; ++i) wc[i] = whh[((size_t)dir * 512 + 128 * q + i) * 128 + k];
  part[q][k] = 0.f;
  float dc = 0.f;
  __syncthreads();
  for (int step = S - 1; step >= 0; --step) {
    const int s = dir ? S - 1 - step : step;
    const int sp = dir ? s + 1 : s - 1;  // the step before s in the forward's order (valid when step > 0)
    if (t < 128) {
      const float dht = dh[((size_t)b * S + s) * 256 + dir * 128 + t] + ((part[0][t] + part[1][t]) + (part[2][t] + part[3][t]));
      const size_t r = ((size_t)b * 2 + dir) * S + s;
      const float* gs = gates + r * 512 + t;
      const float ig = gs[0], fg = gs[128], gg = gs[256], og = gs[384];
      const float c = cst[r * 128 + t];
      const float cp = step > 0 ? cst[(((size_t)b * 2 + dir) * S + sp) * 128 + t] : 0.f;
      const float tc = tanhf(c);
      const float dct = dc + dht * og * (1.f - tc * tc);
      const float d_i = dct * gg * ig * (1.f - ig);
      const float d_f = dct * cp * fg * (1.f - fg);
      const float d_g = dct * ig * (1.f - gg * gg);
      const float d_o = dht * tc * og * (1.f - og);
      dc = dct * fg;
      dgl[t] = d_i, dgl[128 + t] = d_f, dgl[256 + t] = d_g, dgl[384 + t] = d_o;
      const size_t row = ((size_t)dir * B + b) * S + s;
      float* dg = dgates + row * 512 + t;
      dg[0] = d_i, dg[128] = d_f, dg[256] = d_g, dg[384] = d_o;
      hprev[row * 128 + t] = step > 0 ? hout[((size_t)b * S + sp) * 256 + dir * 128 + t] : 0.f;
    }
    __syncthreads();
    if (step > 0) {
      float acc = 0.f;
      const float* dq = dgl + 128 * q;
#pragma unroll
      for (int i = 0; i < 128; i += 4) {
        const f32x4 v = *(const f32x4*)&dq[i];
        acc = fmaf(wc[i], v[0], acc);
        acc = fmaf(wc[i + 1], v[1], acc);
        acc = fmaf(wc[i + 2], v[2], acc);
        acc = fmaf(wc[i + 3], v[3], acc);
      }
      part[q][k] = acc;
    }
    __syncthreads();
  }
}

// dst[z][i] = sum_s src[z][s][i]  (slab sums; the LSTM bias gradient over the (b, s) rows); grid (n / 32, z)
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* src, int nslab, long long stride, long long zstride,
                                                       int n, float* dst) {
  __shared__ float red[8][32];
  const int l = threadIdx.x & 31, part = threadIdx.x >> 5;  // 32 destinations x 8 interleaved slab ranges
  const int i = blockIdx.x * 32 + l;
  float acc = 0.f;
  if (i < n) {
    const float* p = src + blockIdx.y * zstride + i;
    for (int s = part; s < nslab; s += 8) acc += p[(size_t)s * stride];
  }
  red[part][l] = acc;
  __syncthreads();
  if (part == 0 && i < n) {
#pragma unroll
    for (int k = 1; k < 8; ++k) acc += red[k][l];
    dst[(size_t)blockIdx.y * n + i] = acc;
  }
}

// ------------------------------------------------------------------------------------------ time convs
// acc[j] += g x[p + j] / out[p + j] += g w[j] with a wave-uniform winner p: a uniform branch per position keeps
// every register index static.
template <int KW>
SNRSE_DEV void tc_gather(float (&acc)[KW], const float (&x)[8], float g, int p) {
#pragma unroll
  for (int pp = 0; pp < 9 - KW; ++pp)
    if (p == pp) {
#pragma unroll
      for (int j = 0; j < KW; ++j) acc[j] = fmaf(g, x[pp + j], acc[j]);
    }
}
template <int KW>
SNRSE_DEV void tc_scatter(float (&out)[8], const float (&w)[KW], float g, int p) {
#pragma unroll
  for (int pp = 0; pp < 9 - KW; ++pp)
    if (p == pp) {
#pragma unroll
      for (int j = 0; j < KW; ++j) out[pp + j] = fmaf(g, w[j], out[pp + j]);
    }
}

// dW_k[co][ci][fh][j] = sum_n g(n, k, co) a2[n][ci][fh][p*(n, k, co) + j]; db_k[co] = sum_n g.
// grid (ci, co / 4); wave = one co, lane = fh; the thread owns its 15 destinations (all four convs) and walks n.
__global__ __launch_bounds__(256) void timeconv_wgrad_kernel(const float* a2, const float* dfeat, const uint8_t* winp,
                                                             int N, float* dw1, float* dw2, float* dw3, float* dw4,
                                                             float* db1, float* db2, float* db3, float* db4) {
  const int ci = blockIdx.x, tid = threadIdx.x;
  const int co = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(tid >> 6), fh = tid & 63;
  float a1[1] = {0.f}, a2_[2] = {0.f, 0.f}, a4[4] = {0.f, 0.f, 0.f, 0.f}, a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < N; ++n) {
    float x[8];
    const float* xr = a2 + (((size_t)n * 32 + ci) * 64 + fh) * 8;
    *(f32x4*)&x[0] = *(const f32x4*)xr;
    *(f32x4*)&x[4] = *(const f32x4*)(xr + 4);
    const size_t o = (size_t)n * 128 + co;
    const float g0 = dfeat[o], g1 = dfeat[o + 32], g2 = dfeat[o + 64], g3 = dfeat[o + 96];
    const int p0 = __builtin_amdgcn_readfirstlane(winp[o]), p1 = __builtin_amdgcn_readfirstlane(winp[o + 32]),
              p2 = __builtin_amdgcn_readfirstlane(winp[o + 64]);
    tc_gather<1>(a1, x, g0, p0);
    tc_gather<2>(a2_, x, g1, p1);
    tc_gather<4>(a4, x, g2, p2);
    tc_gather<8>(a8, x, g3, 0);
    bs[0] += g0, bs[1] += g1, bs[2] += g2, bs[3] += g3;
  }
  const size_t r = ((size_t)co * 32 + ci) * 64 + fh;
  dw1[r] = a1[0];
  dw2[r * 2] = a2_[0], dw2[r * 2 + 1] = a2_[1];
  *(f32x4*)&dw3[r * 4] = f32x4{a4[0], a4[1], a4[2], a4[3]};
  *(f32x4*)&dw4[r * 8] = f32x4{a8[0], a8[1], a8[2], a8[3]};
  *(f32x4*)&dw4[r * 8 + 4] = f32x4{a8[4], a8[5], a8[6], a8[7]};
  if (ci == 0 && fh == 0) db1[co] = bs[0], db2[co] = bs[1], db3[co] = bs[2], db4[co] = bs[3];
}

template <int KW>
SNRSE_DEV void tc_dgrad_conv(float (&out)[8], const float* w, const float* dfeat, const uint8_t* winp, size_t o,
                             int ci, int fh) {
  for (int co = 0; co < 32; ++co) {
    const float g = dfeat[o + co];
    const int p = KW == 8 ? 0 : __builtin_amdgcn_readfirstlane(winp[o + co]);
    float wt[KW];
    const float* wr = w + (((size_t)co * 32 + ci) * 64 + fh) * KW;
#pragma unroll
    for (int j = 0; j < KW; ++j) wt[j] = wr[j];
    tc_scatter<KW>(out, wt, g, p);
  }
}

// da2[n][ci][fh][t] = sum_{k, co} g(n, k, co) W_k[co][ci][fh][t - p*]; grid (n, ci / 4); wave = ci, lane = fh
__global__ __launch_bounds__(256) void timeconv_dgrad_kernel(const float* dfeat, const uint8_t* winp, const float* w1,
                                                             const float* w2, const float* w3, const float* w4,
                                                             float* da2) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const int ci = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(tid >> 6), fh = tid & 63;
  float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const size_t o = (size_t)n * 128;
  tc_dgrad_conv<1>(out, w1, dfeat, winp, o, ci, fh);
  tc_dgrad_conv<2>(out, w2, dfeat, winp, o + 32, ci, fh);
  tc_dgrad_conv<4>(out, w3, dfeat, winp, o + 64, ci, fh);
  tc_dgrad_conv<8>(out, w4, dfeat, winp, o + 96, ci, fh);
  float* d = da2 + (((size_t)n * 32 + ci) * 64 + fh) * 8;
  *(f32x4*)d = f32x4{out[0], out[1], out[2], out[3]};
  *(f32x4*)(d + 4) = f32x4{out[4], out[5], out[6], out[7]};
}

// ------------------------------------------------------------------------------------------ conv3x3 backward
// dgrad: da1[n][ci][f][t] = sum_{co, dy, dx} W3[co][ci][dy][dx] dy3[n][co][f + 1 - dy][t + 1 - dx], where dy3 is
// da2 routed to the (2, 1) pool's winner.  conv3_pool_kernel's tiling with the roles of ci / co swapped and the
// taps flipped: block = (chunk, 32 rows), lane = (4 rows, frame), wave w: input channels 8 w + [0, 8); the
// routed gradient of 8 output channels is staged per step.
__global__ __launch_bounds__(256) void conv3_dgrad_kernel(const float* da2, const uint8_t* win2, const float* w,
                                                          float* da1) {
  __shared__ float xs[C3_CK][C3_IR][C3_IC];
  __shared__ __attribute__((aligned(16))) float ws[32][C3_CK][12];  // [ci][co][9 flipped taps padded to 12]
  const int tid = threadIdx.x;
  const int n = blockIdx.x >> 2, ft = blockIdx.x & 3;
  const int f0 = ft * 32;
  const float* src = da2 + (size_t)n * 32 * 64 * 8;
  const uint8_t* wsrc = win2 + (size_t)n * 32 * 64 * 8;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int fp = lane >> 3, t = lane & 7;
  const int cb = 8 * wid;
  float acc[8][4];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[c][r] = 0.f;
  for (int c0 = 0; c0 < 32; c0 += C3_CK) {
    __syncthreads();
    for (int i = tid; i < C3_CK * C3_IR * C3_IC; i += 256) {
      const int co = i / (C3_IR * C3_IC), rem = i - co * (C3_IR * C3_IC);
      const int r = rem / C3_IC, c = rem - r * C3_IC;
      const int f = f0 + r - 1, tt = c - 1;
      float v = 0.f;
      if (f >= 0 && f < 128 && tt >= 0 && tt < 8) {
        const int idx = ((c0 + co) * 64 + (f >> 1)) * 8 + tt;
        if (wsrc[idx] == (f & 1)) v = src[idx];
      }
      xs[co][r][c] = v;
    }
    for (int i = tid; i < 32 * C3_CK * 12; i += 256) {
      const int ci = i / (C3_CK * 12), rem = i - ci * (C3_CK * 12), co = rem / 12, tap = rem - co * 12;
      ws[ci][co][tap] = tap < 9 ? w[((c0 + co) * 32 + ci) * 9 + (8 - tap)] : 0.f;
    }
    __syncthreads();
    for (int co = 0; co < C3_CK; ++co) {
      float px[6][3];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) px[r][c] = xs[co][4 * fp + r][t + c];
#pragma unroll 2
      for (int c = 0; c < 8; ++c) {
        float wt[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) *(f32x4*)&wt[4 * q] = *(const f32x4*)&ws[cb + c][co][4 * q];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[c][r] = fmaf(wt[dy * 3 + dx], px[r + dy][dx], acc[c][r]);
      }
    }
  }
  float* o = da1 + (size_t)n * 32 * 128 * 8 + (size_t)(f0 + 4 * fp) * 8 + t;
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(size_t)(cb + c) * 128 * 8 + r * 8] = acc[c][r];
}

// wgrad: dW3[co][ci][dy][dx] = sum over the pooled positions (n, fp, t) of da2[n][co][fp][t] *
// a1[n][ci][2 fp + win + dy - 1][t + dx - 1]; db3[co] = sum da2.  Work unit = (chunk, 16 a1 rows = 8 pooled rows);
// a workgroup walks its units with the a1 tile, the gradients and the winners of the unit in LDS.  Thread =
// (ci, 4 output channels): 36 + 4 sums in registers over all its units, then its slab.
constexpr int W3_XS = 18 * 10 + 1;  // a1 tile per ci: 18 rows x 10 columns (pad 1), + 1: ci lanes on distinct banks
__global__ __launch_bounds__(256) void conv3_wgrad_kernel(const float* a1, const float* da2, const uint8_t* win2,
                                                          int units, float* slabs) {
  __shared__ float xs[32 * W3_XS];
  __shared__ float gs[32][64];
  __shared__ uint8_t wn[32][64];
  const int tid = threadIdx.x, ci = tid & 31, cog = tid >> 5;
  float acc[4][9], bacc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bacc[q] = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[q][k] = 0.f;
  }
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int n = u >> 3, f0 = (u & 7) * 16;
    __syncthreads();
    for (int i = tid; i < 32 * 180; i += 256) {
      const int c = i / 180, rem = i - c * 180, r = rem / 10, col = rem - r * 10;
      const int f = f0 + r - 1, tt = col - 1;
      xs[c * W3_XS + rem] = (f >= 0 && f < 128 && tt >= 0 && tt < 8) ? a1[(((size_t)n * 32 + c) * 128 + f) * 8 + tt] : 0.f;
    }
    for (int i = tid; i < 32 * 64; i += 256) {
      const int c = i >> 6, pos = i & 63;
      const size_t idx = (((size_t)n * 32 + c) * 64 + (f0 >> 1)) * 8 + pos;
      gs[c][pos] = da2[idx];
      wn[c][pos] = win2[idx];
    }
    __syncthreads();
    for (int pos = 0; pos < 64; ++pos) {
      const int fpl = pos >> 3, t = pos & 7;
      float patch[4][3];
      const float* xp = xs + ci * W3_XS + (2 * fpl) * 10 + t;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) patch[r][c] = xp[r * 10 + c];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float g = gs[cog * 4 + q][pos];
        const bool hi = wn[cog * 4 + q][pos] != 0;
        bacc[q] += g;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx)
            acc[q][dy * 3 + dx] = fmaf(g, hi ? patch[dy + 1][dx] : patch[dy][dx], acc[q][dy * 3 + dx]);
      }
    }
  }
  float* sl = slabs + (size_t)blockIdx.x * SLAB;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int co = cog * 4 + q;
#pragma unroll
    for (int k = 0; k < 9; ++k) sl[(co * 32 + ci) * 9 + k] = acc[q][k];
    if (ci == 0) sl[32 * 32 * 9 + co] = bacc[q];
  }
}

// ------------------------------------------------------------------------------------------ conv5x5 backward
// dW5[co][ci][dy][dx] = sum over the pooled positions (n, fo, to) of da1[n][co][fo][to] *
// x[n][ci][2 fo + py + dy - 2][2 to + qx + dx - 2], (py, qx) the 2x2 winner; db5[co] = sum da1.  Work unit =
// (chunk, 32 spectrogram rows), staged as conv5_pool_kernel stages them (read in place).  Thread = (co, 1/8 of
// the 50 taps): 7 sums in registers, then its slab.
__global__ __launch_bounds__(256) void conv5_wgrad_kernel(const float2* spec, int T, const float* da1,
                                                          const uint8_t* win1, int units, float* slabs) {
  __shared__ float xs[2 * C5_IR * C5_IC];
  __shared__ float gs[32][128];
  __shared__ uint8_t wn[32][128];
  const int tid = threadIdx.x, co = tid >> 3, sub = tid & 7;
  const int S = T / 16;
  int off[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int tap = min(sub + 8 * k, 49);
    const int c = tap / 25, rem = tap - c * 25, dy = rem / 5, dx = rem - dy * 5;
    off[k] = (c * C5_IR + dy) * C5_IC + dx;
  }
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int n = u >> 3, f0 = (u & 7) * C5_FT;
    const int b = n / S, k = n - b * S;
    const float2* base = spec + (size_t)b * 256 * T + k * 16;
    __syncthreads();
    for (int i = tid; i < C5_IR * C5_IC; i += 256) {
      const int r = i / C5_IC, c = i - r * C5_IC;
      const int f = f0 + r - 2, t = c - 2;
      float2 v = make_float2(0.f, 0.f);
      if (f >= 0 && f < 256 && t >= 0 && t < 16) v = base[(size_t)f * T + t];
      xs[i] = v.x;
      xs[C5_IR * C5_IC + i] = v.y;
    }
    for (int i = tid; i < 32 * 128; i += 256) {
      const int c = i >> 7, pos = i & 127;
      const size_t idx = (((size_t)n * 32 + c) * 128 + (f0 >> 1)) * 8 + pos;
      gs[c][pos] = da1[idx];
      wn[c][pos] = win1[idx];
    }
    __syncthreads();
    for (int pos = 0; pos < 128; ++pos) {
      const float g = gs[co][pos];
      const int wv = wn[co][pos];
      const float* xp = xs + (2 * (pos >> 3) + (wv >> 1)) * C5_IC + 2 * (pos & 7) + (wv & 1);
      bacc += g;
#pragma unroll
      for (int k = 0; k < 7; ++k) acc[k] = fmaf(g, xp[off[k]], acc[k]);
    }
  }
  float* sl = slabs + (size_t)blockIdx.x * SLAB;
#pragma unroll
  for (int k = 0; k < 7; ++k)
    if (sub + 8 * k < 50) sl[co * 50 + sub + 8 * k] = acc[k];
  if (sub == 0) sl[1600 + co] = bacc;
}

}  // namespace

extern "C" size_t snrse_snrnet_train_workspace(int B, int T) {
  if (B <= 0 || T < 32 || T % 16) return 0;
  return layout(B, T).bytes;
}

extern "C" int snrse_snr_perturb(const void* x, const void* y, const float* gt, int B, long long per, void* out,
                                 hipStream_t s) {
  if (!x || !y || !gt || !out || B <= 0 || per <= 0) return SNRSE_EINVAL;
  const long long n = (long long)B * per;
  hipLaunchKernelGGL(snr_perturb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float2*)x,
                     (const float2*)y, gt, per, n, (float2*)out);
  return (int)hipGetLastError();
}

// Weights as snrse_snrnet; tws: snrse_snrnet_train_workspace(B, T) bytes, kept by the caller until the backward.
extern "C" int snrse_snrnet_train_fwd(const void* spec, int B, int T, const float* w5, const float* b5,
                                      const float* w3, const float* b3, const float* wt1, const float* wt2,
                                      const float* wt3, const float* wt4, const float* bt1, const float* bt2,
                                      const float* bt3, const float* bt4, const float* wih, const float* bsum,
                                      const float* whh, const float* fcw, const float* fcb, void* tws, float* out,
                                      hipStream_t s) {
  if (B <= 0 || T < 32 || T % 16 || !spec || !tws || !out) return SNRSE_EINVAL;
  const int S = T / 16, N = B * S;
  const Layout L = layout(B, T);
  char* base = (char*)tws;
  float* a1 = (float*)(base + L.a1);
  float* a2 = (float*)(base + L.a2);
  float* feat = (float*)(base + L.feat);
  float* xg = (float*)(base + L.xg);
  float* hout = (float*)(base + L.hout);
  hipLaunchKernelGGL(conv5_pool_kernel<true>, dim3(N * 8), dim3(256), 0, s, (const float2*)spec, T, w5, b5, a1, N,
                     (uint8_t*)(base + L.win1));
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv3_pool_kernel<true>, dim3(N * 4), dim3(256), 0, s, a1, w3, b3, a2, N,
                     (uint8_t*)(base + L.win2));
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(timeconv_kernel<true>, dim3((N + TC_NB - 1) / TC_NB, 2, 4), dim3(256), 0, s, a2, wt1, wt2, wt3,
                     wt4, bt1, bt2, bt3, bt4, feat, N, (uint8_t*)(base + L.winp));
  SNRSE_LAUNCH_CHECK();
  const int n4 = B * 2 * S * 512;
  hipLaunchKernelGGL(lstm_input_kernel, dim3((n4 + 255) / 256), dim3(256), 0, s, feat, wih, bsum, xg, B, S);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(lstm_rec_kernel<true>, dim3(2 * B), dim3(512), 0, s, xg, whh, hout, S,
                     (float*)(base + L.gates), (float*)(base + L.cst));
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(snr_head_kernel<true>, dim3(B), dim3(256), 0, s, hout, fcw, fcb, out, S, (int*)(base + L.arg));
  return (int)hipGetLastError();
}

// est: the forward's output [B]; dest: d loss / d est [B]; tws: the forward's workspace.  Gradients in the
// packed layout of the weights: dwih / dwhh [2][512][128], dbsum [2][512] (the gradient of b_ih and of b_hh).
extern "C" int snrse_snrnet_backward(const void* spec, int B, int T, const float* est, const float* dest,
                                     const float* w3, const float* wt1, const float* wt2, const float* wt3,
                                     const float* wt4, const float* wih, const float* whh, const float* fcw,
                                     void* tws, float* dw5, float* db5, float* dw3, float* db3, float* dwt1,
                                     float* dwt2, float* dwt3, float* dwt4, float* dbt1, float* dbt2, float* dbt3,
                                     float* dbt4, float* dwih, float* dbsum, float* dwhh, float* dfcw, float* dfcb,
                                     hipStream_t s) {
  if (B <= 0 || T < 32 || T % 16 || !spec || !tws || !est || !dest) return SNRSE_EINVAL;
  const int S = T / 16, N = B * S;
  const Layout L = layout(B, T);
  char* base = (char*)tws;
  const float* a1 = (const float*)(base + L.a1);
  const float* a2 = (const float*)(base + L.a2);
  const float* feat = (const float*)(base + L.feat);
  const float* hout = (const float*)(base + L.hout);
  const uint8_t* win1 = (const uint8_t*)(base + L.win1);
  const uint8_t* win2 = (const uint8_t*)(base + L.win2);
  const uint8_t* winp = (const uint8_t*)(base + L.winp);
  float* dh = (float*)(base + L.dh);
  float* dgates = (float*)(base + L.dgates);
  float* hprev = (float*)(base + L.hprev);
  float* dfeat = (float*)(base + L.dfeat);
  float* da2 = (float*)(base + L.da2);
  float* da1 = (float*)(base + L.da1);
  float* stats = (float*)(base + L.stats);
  float* dz = (float*)(base + L.dz);
  float* slabs = (float*)(base + L.slabs);

  hipLaunchKernelGGL(head_bwd_kernel, dim3(B), dim3(256), 0, s, hout, (const int*)(base + L.arg), fcw, est, dest, S,
                     dh, stats, dz);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_wgrad_kernel, dim3(4), dim3(256), 0, s, stats, dz, B, dfcw, dfcb);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(lstm_bwd_kernel, dim3(2 * B), dim3(512), 0, s, dh, (const float*)(base + L.gates),
                     (const float*)(base + L.cst), hout, whh, B, S, dgates, hprev);
  SNRSE_LAUNCH_CHECK();
  // dW_hh[dir] = dgates[dir]^T h_prev[dir], dW_ih[dir] = dgates[dir]^T feat: reductions over the (b, s) rows
  int rc = snrse_bgemm(dgates, (long long)N * 512, 1, 512, hprev, (long long)N * 128, 128, 1, dwhh, 512 * 128, 128, 1,
                       nullptr, 2, 512, 128, N, 1.f, 0.f, s);
  if (rc) return rc;
  rc = snrse_bgemm(dgates, (long long)N * 512, 1, 512, feat, 0, 128, 1, dwih, 512 * 128, 128, 1, nullptr, 2, 512, 128,
                   N, 1.f, 0.f, s);
  if (rc) return rc;
  hipLaunchKernelGGL(slab_sum_kernel, dim3(16, 2), dim3(256), 0, s, dgates, N, 512LL, (long long)N * 512, 512, dbsum);
  SNRSE_LAUNCH_CHECK();
  // dfeat = dgates[0] W_ih[0] + dgates[1] W_ih[1]
  for (int dir = 0; dir < 2; ++dir) {
    rc = snrse_bgemm(dgates + (size_t)dir * N * 512, 0, 512, 1, wih + (size_t)dir * 512 * 128, 0, 128, 1, dfeat, 0, 128,
                     1, nullptr, 1, N, 128, 512, 1.f, dir ? 1.f : 0.f, s);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(timeconv_wgrad_kernel, dim3(32, 8), dim3(256), 0, s, a2, dfeat, winp, N, dwt1, dwt2, dwt3, dwt4,
                     dbt1, dbt2, dbt3, dbt4);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(timeconv_dgrad_kernel, dim3(N, 8), dim3(256), 0, s, dfeat, winp, wt1, wt2, wt3, wt4, da2);
  SNRSE_LAUNCH_CHECK();
  const int units = N * 8;
  const int nwg = units < WG_SLABS ? units : WG_SLABS;
  hipLaunchKernelGGL(conv3_wgrad_kernel, dim3(nwg), dim3(256), 0, s, a1, da2, win2, units, slabs);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(slab_sum_kernel, dim3(288, 1), dim3(256), 0, s, slabs, nwg, (long long)SLAB, 0LL, 32 * 32 * 9, dw3);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(slab_sum_kernel, dim3(1, 1), dim3(256), 0, s, slabs + 32 * 32 * 9, nwg, (long long)SLAB, 0LL, 32,
                     db3);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv3_dgrad_kernel, dim3(N * 4), dim3(256), 0, s, da2, win2, w3, da1);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv5_wgrad_kernel, dim3(nwg), dim3(256), 0, s, (const float2*)spec, T, da1, win1, units, slabs);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(slab_sum_kernel, dim3(50, 1), dim3(256), 0, s, slabs, nwg, (long long)SLAB, 0LL, 1600, dw5);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(slab_sum_kernel, dim3(1, 1), dim3(256), 0, s, slabs + 1600, nwg, (long long)SLAB, 0LL, 32, db5);
  return (int)hipGetLastError();
}
