// conv_pool.hip -- MaxPool / MeanPool behind a Conv layer of the trunk (Flux / NNlib semantics, which are torch's defaults): the pool's forward and reverse pass on gfx950.
// Included in front of conv.hip, whose drivers (and conv_pair.hip's, conv_group.hip's) insert the two launches.
//
// For conv layer l: Y_l = act(conv) [OW OH cout x B] is what conv.hip's forward kernel writes, P_l = pool(Y_l) [PW PH cout x B] what the next layer (or flatten) reads,
//   PW = floor((OW + 2 pad1 - k1) / stride1) + 1 (likewise PH); trailing rows and columns that no window reaches are dropped; pad symmetric per axis, pad < k.
//   max   padding taps do not take part (every window has a tap inside the image: pad < k); a NaN in the window gives NaN; ties go to the first element in window order, u1
//         (along W) fastest: the scan keeps a value that is strictly greater or a NaN. The chosen offset u1 + k1 u2 goes, one byte, to an index plane beside P_l (k1 k2 <= 256)
//   mean  the sum of the window's taps inside the image in window order, divided by k1 k2 always (NNlib; torch's count_include_pad = True)
// Reverse: dY_l[i] = sum of dP_l[o] over the windows o that chose i (max), or over the windows that contain i, the sum divided once by k1 k2 (mean); dZ_l = act'(Y_l) dY_l.
//
// These layers move data: no reduction over a long index, so neither LDS nor MFMA. The design is addressing and who writes what.
//   k_pool_fwd  one thread per POOLED element, pw fastest, then ph, channel, sample: neighbouring lanes read neighbouring (strided) image columns and write contiguous outputs
//               (value and index byte); the window is scanned u2 outer, u1 inner in registers
//   k_pool_bwd  gather form, as k_conv_dgrad: one thread per element of Y_l walks the at most ceil(k1 / s1) ceil(k2 / s2) windows that contain it in ascending (ph, pw) order
//               and writes dZ_l once, zeros included (elements no window covers get exactly 0): no float atomics, nothing depends on the grid, two calls give the same bits.
//               stride == window and pad == 0: at most one window, found by one division per axis, no loop
// The member of a trunk pair or group is blockIdx.y: the members' pointers travel by value beside ONE descriptor (ConvGroup's arrangement), a single trunk is M = 1. Each
// member therefore meets the single pass's operands in its order: bit-identical per member.
// Compiled without the packed-f32 instructions: every operation below is one scalar f32 operation, as it is written.
#include "common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define CONV_POOL_NOPK __attribute__((target("no-packed-fp32-ops")))
#else
#define CONV_POOL_NOPK
#endif
#define CONV_POOL_NONE 0
#define CONV_POOL_MAX 1
#define CONV_POOL_MEAN 2

// IW, IH: the extent of Y_l (the conv layer's OW, OH); C its channels; act the conv layer's activation
struct ConvPoolDesc { int32_t kind, k1, k2, s1, s2, p1, p2; int32_t IW, IH, C, PW, PH, act; };
struct ConvPoolGroup {
  ConvPoolDesc d; int32_t B;
  const float* y[CRUX_GROUP_MAX];      // Y_l [IW IH C x B]
  float* p[CRUX_GROUP_MAX];            // forward: P_l [PW PH C x B]
  uint8_t* idx[CRUX_GROUP_MAX];        // max: the chosen offset of every pooled element (written forward, read in reverse)
  const float* dp[CRUX_GROUP_MAX];     // reverse: d(loss)/dP_l
  float* dz[CRUX_GROUP_MAX];           // reverse: d(loss)/dZ_l [IW IH C x B]
};

template <int KIND>
__global__ __launch_bounds__(256) CONV_POOL_NOPK void k_pool_fwd(const ConvPoolGroup t) {
  const ConvPoolDesc& d = t.d; const unsigned m = blockIdx.y;
  const int64_t total = (int64_t)t.B * d.C * d.PH * d.PW;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; if (e >= total) return;
  const int pw = (int)(e % d.PW); const int64_t r = e / d.PW; const int ph = (int)(r % d.PH); const int64_t cb = r / d.PH;      // cb = channel + C sample: one image plane
  const float* y = t.y[m] + cb * ((int64_t)d.IW * d.IH);
  const int iw0 = pw * d.s1 - d.p1, ih0 = ph * d.s2 - d.p2;
  float best = 0.f; int arg = -1;
  for (int u2 = 0; u2 < d.k2; ++u2) {
    const int ih = ih0 + u2; if (ih < 0 || ih >= d.IH) continue;
    for (int u1 = 0; u1 < d.k1; ++u1) {
      const int iw = iw0 + u1; if (iw < 0 || iw >= d.IW) continue;
      const float v = y[iw + d.IW * ih];
      if (KIND == CONV_POOL_MAX) { if (arg < 0 || v > best || v != v) { best = v; arg = u1 + d.k1 * u2; } }
      else best += v;
    }
  }
  if (KIND == CONV_POOL_MAX) { t.p[m][e] = best; t.idx[m][e] = (uint8_t)arg; }
  else t.p[m][e] = best / (float)(d.k1 * d.k2);
}

// the windows along one axis that contain image coordinate i: p in [lo, hi] with p s - pad <= i <= p s - pad + k - 1, clipped to the pooled extent
__device__ __forceinline__ void conv_pool_span(const int n, const int k, const int s, const int P, int& lo, int& hi) {      // n = i + pad
  hi = n / s; if (hi > P - 1) hi = P - 1;
  const int t = n - k + 1; lo = t <= 0 ? 0 : (t + s - 1) / s;
}
template <int KIND>
__global__ __launch_bounds__(256) CONV_POOL_NOPK void k_pool_bwd(const ConvPoolGroup t) {
  const ConvPoolDesc& d = t.d; const unsigned m = blockIdx.y;
  const int64_t total = (int64_t)t.B * d.C * d.IH * d.IW;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; if (e >= total) return;
  const int iw = (int)(e % d.IW); const int64_t r = e / d.IW; const int ih = (int)(r % d.IH); const int64_t cb = r / d.IH;
  const int64_t plane = cb * ((int64_t)d.PW * d.PH);
  const float* dp = t.dp[m] + plane; const uint8_t* ix = KIND == CONV_POOL_MAX ? t.idx[m] + plane : nullptr;
  float acc = 0.f;
  if (d.s1 == d.k1 && d.s2 == d.k2 && d.p1 == 0 && d.p2 == 0) {      // the windows tile the image: at most one holds this element
    const int pw = iw / d.s1, ph = ih / d.s2;
    if (pw < d.PW && ph < d.PH) { const int o = pw + d.PW * ph;
      if (KIND != CONV_POOL_MAX || (int)ix[o] == (iw - pw * d.s1) + d.k1 * (ih - ph * d.s2)) acc = dp[o]; }
  } else {
    const int nx = iw + d.p1, ny = ih + d.p2; int wlo, whi, hlo, hhi;
    conv_pool_span(nx, d.k1, d.s1, d.PW, wlo, whi); conv_pool_span(ny, d.k2, d.s2, d.PH, hlo, hhi);
    for (int ph = hlo; ph <= hhi; ++ph) {
      const int u2 = ny - ph * d.s2;
      for (int pw = wlo; pw <= whi; ++pw) { const int u1 = nx - pw * d.s1, o = pw + d.PW * ph;
        if (KIND != CONV_POOL_MAX || (int)ix[o] == u1 + d.k1 * u2) acc += dp[o]; }
    }
  }
  if (KIND == CONV_POOL_MEAN) acc = acc / (float)(d.k1 * d.k2);
  t.dz[m][e] = crux_act_grad(d.act, t.y[m][e], acc);
}

// ---- host side: one launch over the M members whose pointers the caller has filled in -------------------------------------------------------------------------------------
static void conv_pool_launch_fwd(hipStream_t st, const ConvPoolGroup& t, int M) {
  const int64_t total = (int64_t)t.B * t.d.C * t.d.PH * t.d.PW; const dim3 grid((unsigned)((total + 255) / 256), (unsigned)M), block(256);
  if (t.d.kind == CONV_POOL_MAX) hipLaunchKernelGGL((k_pool_fwd<CONV_POOL_MAX>), grid, block, 0, st, t);
  else hipLaunchKernelGGL((k_pool_fwd<CONV_POOL_MEAN>), grid, block, 0, st, t);
}
static void conv_pool_launch_bwd(hipStream_t st, const ConvPoolGroup& t, int M) {
  const int64_t total = (int64_t)t.B * t.d.C * t.d.IH * t.d.IW; const dim3 grid((unsigned)((total + 255) / 256), (unsigned)M), block(256);
  if (t.d.kind == CONV_POOL_MAX) hipLaunchKernelGGL((k_pool_bwd<CONV_POOL_MAX>), grid, block, 0, st, t);
  else hipLaunchKernelGGL((k_pool_bwd<CONV_POOL_MEAN>), grid, block, 0, st, t);
}
