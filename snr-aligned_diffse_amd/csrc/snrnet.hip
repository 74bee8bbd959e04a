// SNR estimator (SNRNet, reference sgmse/backbones/snrnet.py:47-97) on gfx950, fp32.
//
// Input: the raw complex STFT of y / max|y| (model.py:715-720) as interleaved complex64
// [B, 256, T] (T a multiple of 16, pad_spec_16) — channel 0 = real, 1 = imag, read in place
// (no view_as_real / permute copies).  Per 16-frame chunk n = b*(T/16) + k:
//   K1 conv5x5(2->32, pad 2) + maxpool 2x2            -> [N, 32, 128, 8]
//   K2 conv3x3(32->32, pad 1) + maxpool (2,1)          -> [N, 32, 64, 8]
//   K3 convt_{1..4} (64 x {1,2,4,8}) + full max-pool   -> feat [N, 128]
//   K4a LSTM input projections, both directions         -> xg [B, 2, S, 512]
//   K4b bidirectional LSTM recurrence (hidden 128)      -> h [B, S, 256]
//   K4c mean / std (unbiased) / min / max over S, FC, sigmoid -> [B]
// Tiny next to one score-network NFE (~1.2 GFLOP per 4 s clip); run once per utterance.
// The stage kernels live in snrnet_stages.h (shared with the training forward, snrnet_train.hip).
#include "snrnet_stages.h"

// Weights (fp32, torch layouts): w5 [32,2,5,5] b5; w3 [32,32,3,3] b3; wt1..4 [32,32,64,kw] bt1..4;
// wih [2][512][128] (forward, reverse), bsum [2][512] = b_ih + b_hh; whh [2][512][128];
// fcw [1024], fcb [1].  Workspace: ws >= N*32*128*8 + N*32*64*8 + N*128 + B*2*S*512 + B*S*256
// floats, N = B*T/16, S = T/16.
extern "C" int snrse_snrnet(const void* spec, int B, int T, const float* w5, const float* b5, const float* w3,
                            const float* b3, const float* wt1, const float* wt2, const float* wt3,
                            const float* wt4, const float* bt1, const float* bt2, const float* bt3,
                            const float* bt4, const float* wih, const float* bsum, const float* whh,
                            const float* fcw, const float* fcb, float* ws, float* out, hipStream_t s) {
  if (B <= 0 || T < 16 || T % 16 || !spec || !ws || !out) return SNRSE_EINVAL;
  const int S = T / 16, N = B * S;
  float* a1 = ws;
  float* a2 = a1 + (size_t)N * 32 * 128 * 8;
  float* feat = a2 + (size_t)N * 32 * 64 * 8;
  float* xg = feat + (size_t)N * 128;
  float* hout = xg + (size_t)B * 2 * S * 512;
  const int n1 = N * 32 * 128 * 8, n2 = N * 32 * 64 * 8;
  (void)n1;
  (void)n2;
  hipLaunchKernelGGL(conv5_pool_kernel<false>, dim3(N * 8), dim3(256), 0, s, (const float2*)spec, T, w5, b5, a1, N,
                     nullptr);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv3_pool_kernel<false>, dim3(N * 4), dim3(256), 0, s, a1, w3, b3, a2, N, nullptr);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(timeconv_kernel<false>, dim3((N + TC_NB - 1) / TC_NB, 2, 4), dim3(256), 0, s, a2, wt1, wt2, wt3,
                     wt4, bt1, bt2, bt3, bt4, feat, N, nullptr);
  SNRSE_LAUNCH_CHECK();
  const int n4 = B * 2 * S * 512;
  hipLaunchKernelGGL(lstm_input_kernel, dim3((n4 + 255) / 256), dim3(256), 0, s, feat, wih, bsum, xg, B, S);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(lstm_rec_kernel<false>, dim3(2 * B), dim3(512), 0, s, xg, whh, hout, S, nullptr, nullptr);
  SNRSE_LAUNCH_CHECK();
  hipLaunchKernelGGL(snr_head_kernel<false>, dim3(B), dim3(256), 0, s, hout, fcw, fcb, out, S, nullptr);
  return (int)hipGetLastError();
}

extern "C" size_t snrse_snrnet_workspace(int B, int T) {
  const size_t S = T / 16, N = (size_t)B * S;
  return sizeof(float) * (N * 32 * 128 * 8 + N * 32 * 64 * 8 + N * 128 + (size_t)B * 2 * S * 512 + B * S * 256);
}
