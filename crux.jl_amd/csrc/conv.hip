// conv.hip -- a convolutional trunk Chain([x -> c x,] Conv..., flatten) in front of the dense engine, on gfx950 f32 MFMA: forward with cached activations, the reverse pass
// (weight / bias gradients, input gradient), and DQN's target and td_loss step over trunk + dense head (examples/rl/atari.jl of the reference: DiscreteNetwork(Chain(x -> x ./ 255f0,
// Conv((8,8), 4=>16, relu, stride=4), Conv((4,4), 16=>32, relu, stride=2), flatten, Dense(2048, 256, relu), Dense(256, n)), as) under DQN).
//
// Semantics are Flux's. Images are WHCN column-major (one sample's features contiguous: w + W (h + H c)); a layer's weights are (k1, k2, cin, cout) column-major followed by its
// cout biases, layer after layer (Flux.params order); Conv is a TRUE convolution (NNlib flips the kernel):
//   y[ow, oh, co] = act(b[co] + sum_{t1, t2, ci} w[t1, t2, ci, co] x[ow s1 - p1 + (k1 - 1 - t1), oh s2 - p2 + (k2 - 1 - t2), ci]),   OW = floor((W + 2 p1 - k1) / s1) + 1
// and flatten keeps that order (ow + OW (oh + OH co)). The kernels walk the FLIPPED taps u1 = k1 - 1 - t1, u2 = k2 - 1 - t2, so the image is read ascending and the flip is an
// index permutation on the weight side (dense.hip: any k permutation is legal as long as both operands agree).
//
// dense.hip's conventions: v_mfma_f32_16x16x4_f32 (exact f32 products, one fma chain per output element), one wave per 16x16 output tile, the reduction index ascending in
// steps of 64 with the loads of the next step in flight, lane group g taking k = 16 q + 4 g + r for MFMA r; no float atomics, no dependence on the grid. No column matrix is
// materialised: the patch operand's address is generated from (k, column) in the load, padding taps are masked to zero.
//   forward  M = cout  N = B OH OW   K = cin k1 k2     k = u1 + k1 (u2 + k2 ci)
//   weights  M = cout  N = cin k1 k2 reduction over the B OH OW columns n = ow + OW (oh + OH b), cut into chunks of CONV_WG_CHUNK columns (a compile-time constant): one wave per
//            (tile, chunk) stores its partial tile, a second launch adds the chunks in chunk order and scales; db rides along as the row sum of the first column tile
//   data     M = cin   N = B IH IW   K = cout k1 k2    k = u1 + k1 (u2 + k2 co), gather form: input element (iw, ih) takes tap u1 of output column ow = (iw + p1 - u1) / s1 when
//            that divides and lies inside; elements no window covers sum nothing and get exactly 0; times act' of the layer that produced the input (its cached output)
// Parameters, gradients and Adam state live in a bare-vector crux_mlp (n_layers = 0) the caller passes in: Adam, copy, polyak and the accessors are the existing entries.
#include "common.h"
#include "exec.h"
#include "ops_small.h"

#define CRUX_CONV_MAXL 4
#define CONV_WG_CHUNK 512      // columns of one weight-gradient partial: a constant, so the sums do not depend on the grid or the card

struct ConvLayerDesc { int32_t k1, k2, cin, cout, s1, s2, p1, p2, act; int32_t IW, IH, OW, OH; int32_t woff, boff, K; };
struct crux_conv {
  crux_ctx* ctx = nullptr;
  int32_t L = 0, W = 0, H = 0, C = 0; float scale = 1.f;
  ConvLayerDesc ly[CRUX_CONV_MAXL];
  int64_t n_params = 0, in_features = 0, feat[CRUX_CONV_MAXL + 1] = {0}, maxfeat = 0;      // feat[l]: features of one sample entering layer l (feat[L]: the flattened output)
  float* ws = nullptr; int64_t ws_B = 0;      // cached outputs of layers 1..L, two delta buffers, the weight-gradient partials; capacity ws_B samples
};

struct ConvArgs {
  ConvLayerDesc d; int32_t B;
  const float* w; const float* bias;
  const float* x; float xscale;           // the layer's input [IW IH cin x B] (forward, weights); multiplied by xscale in the load (the x -> c x prelude of layer 0)
  float* y;                               // forward: act(z) [OW OH cout x B]
  const float* dz;                        // weights, data: d(loss)/dz of this layer [OW OH cout x B]
  float* part;                            // weights: partial tiles [chunk][K cout + cout]
  float* dx; const float* ysrc; int32_t act_prev; float dxscale;      // data: the gradient of the layer's input, act' from ysrc (NULL: times dxscale instead)
};

// one step of 64 reduction indices: sixteen MFMAs on the two register sets of dense.hip's Gemm16
__device__ __forceinline__ void conv_mfma64(const float (&a)[4][4], const float (&b)[4][4], f32x4& acc) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][r], b[u][r], acc, 0, 0, 0);
}
#define CONV_KLOOP(kbeg, kend, load, compute)                                          \
  if ((kbeg) < (kend)) {                                                                \
    float a0[4][4], b0[4][4], a1[4][4], b1[4][4];                                       \
    int64_t k0 = (kbeg); load(k0, a0, b0);                                              \
    for (;;) {                                                                          \
      bool more = k0 + 64 < (kend); if (more) load(k0 + 64, a1, b1);                    \
      compute(a0, b0);                                                                  \
      if (!more) break; k0 += 64;                                                       \
      more = k0 + 64 < (kend); if (more) load(k0 + 64, a0, b0);                         \
      compute(a1, b1);                                                                  \
      if (!more) break; k0 += 64;                                                       \
    }                                                                                   \
  }

// VEC: k1 % 4 == 0, s1 % 4 == 0, p1 == 0, IW % 4 == 0 and both bases 16-byte aligned (conv_fwd_vec): four consecutive k share (u2, ci) and are four consecutive, aligned image
// elements and four consecutive (descending) weights -- one 16-byte load each. Which k meets which is unchanged, so the bits do not depend on the form.
template <bool VEC>
__global__ __launch_bounds__(256) void k_conv_fwd(const ConvArgs q) {
  const ConvLayerDesc& d = q.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int OHW = d.OW * d.OH; const int64_t N = (int64_t)q.B * OHW;
  const int tm = (d.cout + 15) >> 4; const int64_t tn = (N + 15) >> 4;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
  if (tile >= tm * tn) return;
  const int i0 = (int)(tile % tm) << 4; const int64_t j0 = (tile / tm) << 4;
  const int ia = i0 + c; const int64_t jb = j0 + c;
  const bool va = ia < d.cout, vb = jb < N;
  const int64_t jn = vb ? jb : 0; const int b = (int)(jn / OHW), sp = (int)(jn - (int64_t)b * OHW), oh = sp / d.OW, ow = sp - oh * d.OW;
  const int iw0 = ow * d.s1 - d.p1, ih0 = oh * d.s2 - d.p2, K = d.K, k12 = d.k1 * d.k2;
  const float* px = q.x + (int64_t)b * d.IW * d.IH * d.cin;
  const float* pw = q.w + (int64_t)(va ? ia : 0) * K;
  const float xs = q.xscale;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](const int64_t k0, float (&a)[4][4], float (&bq)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kb = (int)k0 + 16 * u + 4 * g;
      int ci = kb / k12; const int rem = kb - ci * k12; int u2 = rem / d.k1, u1 = rem - u2 * d.k1;
      if (VEC) {
        f32x4 ta = {0.f, 0.f, 0.f, 0.f}, tb = {0.f, 0.f, 0.f, 0.f};
        const int ih = ih0 + u2;
        if (va && kb < K) ta = *(const f32x4*)(pw + (d.k1 - 4 - u1) + d.k1 * ((d.k2 - 1 - u2) + d.k2 * ci));
        if (vb && kb < K && ih >= 0 && ih < d.IH) tb = *(const f32x4*)(px + (iw0 + u1) + d.IW * (ih + d.IH * ci));
#pragma unroll
        for (int r = 0; r < 4; ++r) { a[u][r] = ta[3 - r]; bq[u][r] = tb[r] * xs; }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool vk = kb + r < K; const int iw = iw0 + u1, ih = ih0 + u2;
          a[u][r] = (va && vk) ? pw[(d.k1 - 1 - u1) + d.k1 * ((d.k2 - 1 - u2) + d.k2 * ci)] : 0.f;
          bq[u][r] = (vb && vk && iw >= 0 && iw < d.IW && ih >= 0 && ih < d.IH) ? px[iw + d.IW * (ih + d.IH * ci)] * xs : 0.f;
          if (++u1 == d.k1) { u1 = 0; if (++u2 == d.k2) { u2 = 0; ++ci; } }
        }
      }
    } };
  auto compute = [&](const float (&a)[4][4], const float (&bq)[4][4]) { conv_mfma64(a, bq, acc); };
  CONV_KLOOP(0, K, load, compute)
  if (!vb) return;      // D layout: reg r <-> row i0 + 4 g + r, column j0 + c
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int i = i0 + 4 * g + r; if (i >= d.cout) continue;
    q.y[sp + (int64_t)OHW * (i + (int64_t)d.cout * b)] = crux_act(d.act, acc[r] + q.bias[i]); }
}

// weight gradient: wave (tile, chunk) sums dz[co, n] x[patch(kk, n)] over the chunk's columns n ascending; kk is the weight's own (unflipped) index t1 + k1 (t2 + k2 ci)
__global__ __launch_bounds__(256) void k_conv_wgrad(const ConvArgs q) {
  const ConvLayerDesc& d = q.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int OHW = d.OW * d.OH, K = d.K; const int64_t N = (int64_t)q.B * OHW;
  const int tm = (d.cout + 15) >> 4, tk = (K + 15) >> 4, ntile = tm * tk; const int64_t nch = (N + CONV_WG_CHUNK - 1) / CONV_WG_CHUNK;
  const int64_t wid = (int64_t)blockIdx.x * 4 + wv;
  if (wid >= ntile * nch) return;
  const int tile = (int)(wid % ntile); const int64_t ch = wid / ntile;
  const int i0 = (tile % tm) << 4, j0 = (tile / tm) << 4;
  const int ia = i0 + c, jb = j0 + c;
  const bool va = ia < d.cout, vb = jb < K;
  const int kk = vb ? jb : 0, k12 = d.k1 * d.k2, ci = kk / k12, rem = kk - ci * k12, t2 = rem / d.k1, t1 = rem - t2 * d.k1;
  const int ox = d.k1 - 1 - t1 - d.p1, oy = d.k2 - 1 - t2 - d.p2;      // image position of this tap relative to (ow s1, oh s2)
  const int64_t xs_b = (int64_t)d.IW * d.IH * d.cin, zs_b = (int64_t)OHW * d.cout;
  const float* px = q.x + (int64_t)d.IW * d.IH * ci;
  const float* pz = q.dz + (int64_t)OHW * (va ? ia : 0);
  const float xs = q.xscale;
  const int64_t nbeg = ch * CONV_WG_CHUNK, nend = nbeg + CONV_WG_CHUNK < N ? nbeg + CONV_WG_CHUNK : N;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}; float rowsum = 0.f;
  const bool want_rowsum = j0 == 0;
  auto load = [&](const int64_t n0, float (&a)[4][4], float (&bq)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t nb = n0 + 16 * u + 4 * g;
      int b = (int)(nb / OHW); const int sp0 = (int)(nb - (int64_t)b * OHW); int oh = sp0 / d.OW, ow = sp0 - oh * d.OW;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool vn = nb + r < nend; const int iw = ow * d.s1 + ox, ih = oh * d.s2 + oy;
        a[u][r] = (va && vn) ? pz[(int64_t)b * zs_b + ow + d.OW * oh] : 0.f;
        bq[u][r] = (vb && vn && iw >= 0 && iw < d.IW && ih >= 0 && ih < d.IH) ? px[(int64_t)b * xs_b + iw + d.IW * ih] * xs : 0.f;
        if (++ow == d.OW) { ow = 0; if (++oh == d.OH) { oh = 0; ++b; } }
      }
    } };
  auto compute = [&](const float (&a)[4][4], const float (&bq)[4][4]) {
    conv_mfma64(a, bq, acc);
    if (want_rowsum) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) rowsum += a[u][r];
    } };
  CONV_KLOOP(nbeg, nend, load, compute)
  float* part = q.part + ch * ((int64_t)K * d.cout + d.cout);
  if (want_rowsum) {   // lanes c, c + 16, c + 32, c + 48 hold the four column groups of row i0 + c: fixed-order combine (dense.hip)
    rowsum += __shfl_xor(rowsum, 16, 64); rowsum += __shfl_xor(rowsum, 32, 64);
    if (g == 0 && va) part[(int64_t)K * d.cout + ia] = rowsum;
  }
  if (!vb) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int i = i0 + 4 * g + r; if (i < d.cout) part[jb + (int64_t)K * i] = acc[r]; }
}
// the chunks of one gradient element in chunk order, then the scale: g[woff + e], e over the layer's weights and biases (they are contiguous in the flat vector)
__global__ void k_conv_wgrad_combine(const float* __restrict__ part, int64_t per, int64_t nch, float scale, float* __restrict__ gout) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (e >= per) return;
  float s = part[e];
  for (int64_t ch = 1; ch < nch; ++ch) s += part[ch * per + e];
  gout[e] = scale * s;
}

// data gradient, gather form
__global__ __launch_bounds__(256) void k_conv_dgrad(const ConvArgs q) {
  const ConvLayerDesc& d = q.d;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int IHW = d.IW * d.IH, OHW = d.OW * d.OH; const int64_t N = (int64_t)q.B * IHW;
  const int tm = (d.cin + 15) >> 4; const int64_t tn = (N + 15) >> 4;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
  if (tile >= tm * tn) return;
  const int i0 = (int)(tile % tm) << 4; const int64_t j0 = (tile / tm) << 4;
  const int ia = i0 + c; const int64_t jb = j0 + c;
  const bool va = ia < d.cin, vb = jb < N;
  const int64_t jn = vb ? jb : 0; const int b = (int)(jn / IHW), sp = (int)(jn - (int64_t)b * IHW), ih = sp / d.IW, iw = sp - ih * d.IW;
  const int k12 = d.k1 * d.k2, Kd = d.cout * k12;
  const float* pz = q.dz + (int64_t)b * OHW * d.cout;
  const float* pw = q.w + (int64_t)k12 * (va ? ia : 0);
  const int64_t ws_co = (int64_t)k12 * d.cin;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](const int64_t k0, float (&a)[4][4], float (&bq)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kb = (int)k0 + 16 * u + 4 * g;
      int co = kb / k12; const int rem = kb - co * k12; int u2 = rem / d.k1, u1 = rem - u2 * d.k1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool vk = kb + r < Kd;
        const int nx = iw + d.p1 - u1, ny = ih + d.p2 - u2;
        const int ow = nx / d.s1, oh = ny / d.s2;
        const bool hit = nx >= 0 && ny >= 0 && ow * d.s1 == nx && oh * d.s2 == ny && ow < d.OW && oh < d.OH;
        a[u][r] = (va && vk) ? pw[(d.k1 - 1 - u1) + d.k1 * (d.k2 - 1 - u2) + ws_co * co] : 0.f;
        bq[u][r] = (vb && vk && hit) ? pz[ow + d.OW * oh + (int64_t)OHW * co] : 0.f;
        if (++u1 == d.k1) { u1 = 0; if (++u2 == d.k2) { u2 = 0; ++co; } }
      }
    } };
  auto compute = [&](const float (&a)[4][4], const float (&bq)[4][4]) { conv_mfma64(a, bq, acc); };
  CONV_KLOOP(0, Kd, load, compute)
  if (!vb) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int i = i0 + 4 * g + r; if (i >= d.cin) continue;
    const int64_t e = sp + (int64_t)IHW * (i + (int64_t)d.cin * b);
    q.dx[e] = q.ysrc ? crux_act_grad(q.act_prev, q.ysrc[e], acc[r]) : acc[r] * q.dxscale; }
}

// Flux's glorot_uniform for Conv: U(+-sqrt(6 / (k1 k2 cin + k1 k2 cout))) weights, zero biases. crux_rng.h convention of crux_mlp_init_glorot: weight number n of the
// trunk (counted over the layers' weight arrays in order, biases not counted) is (crux_u32_to_f32(philox(seed, n, stream, CRUX_RNG_INIT).v[0]) - 0.5) * 2 limit
struct ConvInit { int32_t L; int32_t woff[CRUX_CONV_MAXL], boff[CRUX_CONV_MAXL], fan[CRUX_CONV_MAXL]; int64_t n_params; };
__global__ void k_conv_glorot(const ConvInit t, float* __restrict__ p, uint64_t seed, uint32_t stream) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (gid >= t.n_params) return;
  int64_t ctr = 0;
  for (int l = 0; l < t.L; ++l) {
    if (gid >= t.woff[l] && gid < t.boff[l]) {
      const float scale = sqrtf(24.0f / (float)t.fan[l]);
      const crux_u32x4 x = crux_philox(seed, (uint64_t)(ctr + (gid - t.woff[l])), stream, CRUX_RNG_INIT);
      p[gid] = (crux_u32_to_f32(x.v[0]) - 0.5f) * scale; return;
    }
    ctr += t.boff[l] - t.woff[l];
  }
  p[gid] = 0.f;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------------------------
static inline int64_t conv_nch(const crux_conv* v, int l, int64_t B) { return (B * v->ly[l].OW * v->ly[l].OH + CONV_WG_CHUNK - 1) / CONV_WG_CHUNK; }
static inline int64_t conv_per(const crux_conv* v, int l) { return (int64_t)v->ly[l].K * v->ly[l].cout + v->ly[l].cout; }
// the workspace grows once (to a power-of-two capacity) and is re-used at smaller B: every buffer is [features x B] with the features contiguous, so the capacity moves the
// buffers' offsets and nothing a kernel computes
static int32_t conv_ensure_ws(crux_conv* v, int64_t B) {
  if (v->ws && v->ws_B >= B) return CRUX_OK;
  crux_ctx* c = v->ctx;
  if (v->ws) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(v->ws); v->ws = nullptr; v->ws_B = 0; }
  int64_t cap = 32; while (cap < B) cap *= 2;
  size_t tot = 0; for (int l = 1; l <= v->L; ++l) tot += (size_t)v->feat[l] * (size_t)cap;
  tot += 2 * (size_t)v->maxfeat * (size_t)cap;
  size_t part = 0; for (int l = 0; l < v->L; ++l) { const size_t p = (size_t)conv_nch(v, l, cap) * (size_t)conv_per(v, l); if (p > part) part = p; }
  tot += part;
  if (hipMalloc(&v->ws, sizeof(float) * tot + 64) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "conv workspace: hipMalloc(%zu) failed", sizeof(float) * tot);
  v->ws_B = cap; return CRUX_OK;
}
static float* conv_act(crux_conv* v, int l) {      // l in 1..L + 2: the cached output of layer l; L + 1, L + 2 the delta buffers (then the partials)
  size_t off = 0; for (int q = 1; q < l && q <= v->L; ++q) off += (size_t)v->feat[q] * (size_t)v->ws_B;
  if (l > v->L) off += (size_t)(l - v->L - 1) * (size_t)v->maxfeat * (size_t)v->ws_B;
  return v->ws + off;
}
static float* conv_part(crux_conv* v) { return conv_act(v, v->L + 3); }

static int32_t conv_check(const char* who, crux_conv* v, crux_mlp* p, int64_t B) {
  if (!v || !p) return CRUX_EINVAL;
  crux_ctx* c = v->ctx;
  if (p->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the parameter handle belongs to another context", who);
  if (p->nd.L != 0 || p->nd.n_params != v->n_params) return crux_fail(c, CRUX_EINVAL, "%s: the parameter handle must be a bare vector (n_layers = 0) of %lld values, has %d layers and %d", who, (long long)v->n_params, p->nd.L, p->nd.n_params);
  if (B < 1 || B * v->maxfeat > 0x7fffffffll) return crux_fail(c, CRUX_EINVAL, "%s: batch %lld out of range", who, (long long)B);
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: a convolutional trunk is not recordable into a fused sequence", who);
  return CRUX_OK;
}
static inline bool conv_fwd_vec(const ConvLayerDesc& d, const float* w, const float* x) {
  return (d.k1 & 3) == 0 && (d.s1 & 3) == 0 && d.p1 == 0 && (d.IW & 3) == 0 && (((uintptr_t)w) & 15) == 0 && (((uintptr_t)x) & 15) == 0;
}
static int32_t conv_forward_ws(const char* who, crux_conv* v, crux_mlp* p, const float* d_x, int64_t B) {
  int32_t rc = conv_check(who, v, p, B); if (rc) return rc;
  crux_ctx* c = v->ctx; rc = conv_ensure_ws(v, B); if (rc) return rc;
  const float* x = d_x;
  for (int l = 0; l < v->L; ++l) {
    ConvArgs q{}; q.d = v->ly[l]; q.B = (int32_t)B; q.w = p->p + q.d.woff; q.bias = p->p + q.d.boff; q.x = x; q.xscale = l == 0 ? v->scale : 1.f; q.y = conv_act(v, l + 1);
    const int64_t tiles = (int64_t)((q.d.cout + 15) >> 4) * ((B * q.d.OW * q.d.OH + 15) >> 4);
    const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
    if (conv_fwd_vec(q.d, q.w, q.x)) hipLaunchKernelGGL((k_conv_fwd<true>), grid, block, 0, c->stream, q);
    else hipLaunchKernelGGL((k_conv_fwd<false>), grid, block, 0, c->stream, q);
    x = q.y;
  }
  return crux_launch_check(c, "k_conv_fwd");
}
// Reverse pass after conv_forward_ws with the same d_x and parameters. d_dy [out_features x B] is not modified.
static int32_t conv_backward_ws(const char* who, crux_conv* v, crux_mlp* p, const float* d_x, int64_t B, const float* d_dy, float gscale, bool want_g, float* d_dx) {
  int32_t rc = conv_check(who, v, p, B); if (rc) return rc;
  crux_ctx* c = v->ctx;
  if (!v->ws || v->ws_B < B) return crux_fail(c, CRUX_EINVAL, "%s: no cached forward pass for this batch", who);
  const float* dcur = d_dy; float* dnxt = conv_act(v, v->L + 1); float* dspare = conv_act(v, v->L + 2);
  if (v->ly[v->L - 1].act != CRUX_ACT_IDENTITY) {      // dZ_L = act'(Y_L) .* dY
    const int64_t cnt = v->feat[v->L] * B;
    crux_launch<ActGradOp>((unsigned)((cnt + 255) / 256), 256, c->stream, d_dy, (const float*)conv_act(v, v->L), (int)v->ly[v->L - 1].act, cnt, dnxt);
    dcur = dnxt; dnxt = dspare; dspare = const_cast<float*>(dcur);
  }
  for (int l = v->L - 1; l >= 0; --l) {
    ConvArgs q{}; q.d = v->ly[l]; q.B = (int32_t)B; q.w = p->p + q.d.woff; q.x = l == 0 ? d_x : conv_act(v, l); q.xscale = l == 0 ? v->scale : 1.f; q.dz = dcur;
    if (want_g) {
      const int64_t nch = conv_nch(v, l, B), per = conv_per(v, l), waves = nch * ((q.d.cout + 15) >> 4) * ((q.d.K + 15) >> 4);
      q.part = conv_part(v);
      hipLaunchKernelGGL(k_conv_wgrad, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c->stream, q);
      hipLaunchKernelGGL(k_conv_wgrad_combine, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, c->stream, (const float*)q.part, per, nch, gscale, p->g + q.d.woff);
    }
    if (l > 0 || d_dx) {
      q.dx = l > 0 ? dnxt : d_dx; q.ysrc = l > 0 ? q.x : nullptr; q.act_prev = l > 0 ? v->ly[l - 1].act : CRUX_ACT_IDENTITY; q.dxscale = v->scale;
      const int64_t tiles = (int64_t)((q.d.cin + 15) >> 4) * ((B * q.d.IW * q.d.IH + 15) >> 4);
      hipLaunchKernelGGL(k_conv_dgrad, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, c->stream, q);
      dcur = dnxt; float* t = dnxt; dnxt = dspare; dspare = t;
    }
  }
  return crux_launch_check(c, "conv backward");
}

// ---- DQN over trunk + dense head (rl/dqn.jl:4-6, utils.jl:76-87): the trunk's features feed the dense engine's passes, the per-sample arithmetic is crux_td_step's ------------
static int32_t conv_pair_check(const char* who, crux_conv* v, crux_mlp* trunk, crux_mlp* head, crux_buffer* b) {
  if (!v || !trunk || !head || !b) return CRUX_EINVAL;
  crux_ctx* c = v->ctx; const int64_t B = b->elements;
  if (head->ctx != c || b->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: head and batch must belong to the trunk's context", who);
  if (B < 1) return crux_fail(c, CRUX_EINVAL, "%s: empty batch", who);
  int32_t rc = conv_check(who, v, trunk, B); if (rc) return rc;
  if (b->obs_dim != v->in_features) return crux_fail(c, CRUX_EINVAL, "%s: observations have %d features, the trunk takes %lld (W H C)", who, b->obs_dim, (long long)v->in_features);
  if (head->nd.L < 1 || head->nd.dims[0] != v->feat[v->L]) return crux_fail(c, CRUX_EINVAL, "%s: the head must take the trunk's %lld flattened features", who, (long long)v->feat[v->L]);
  if (b->act_kind != CRUX_ACTION_DISCRETE || head->nd.dims[head->nd.L] != b->act_dim) return crux_fail(c, CRUX_EINVAL, "%s: needs a one-hot action column matching the Q outputs", who);
  return CRUX_OK;
}
static int32_t conv_td_step_impl(const char* who, crux_conv* v, crux_mlp* trunk, crux_mlp* head, crux_buffer* b, const float* d_y, int32_t use_weight, float* info_out, float* d_err) {
  if (!d_y) return CRUX_EINVAL;
  int32_t rc = conv_pair_check(who, v, trunk, head, b); if (rc) return rc;
  crux_ctx* c = v->ctx; const int64_t B = b->elements, F = v->feat[v->L]; const int nout = head->nd.dims[head->nd.L];
  if (use_weight && !has_col(b, CRUX_COL_WEIGHT)) return crux_fail(c, CRUX_EINVAL, "%s(weight=:weight): batch has no :weight column", who);
  if (!trunk->has_adam || !head->has_adam) return crux_fail(c, CRUX_EINVAL, "%s: crux_adam_init was not called on both handles", who);
  Carve cv{(char*)crux_scratch(c, 4 * (size_t)B * (size_t)(nout + F) + 8192), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  float* dy = cv.take<float>((size_t)B * nout); float* dfeat = cv.take<float>((size_t)B * (size_t)F); Carve sv = small_carve(c, cv, 256 * 6);
  float* dinfo = sv.take<float>(CRUX_INFO_N); double* st = sv.take<double>(2); double* ssq = sv.take<double>(2 + SUMSQ_BLOCKS); int32_t* status = sv.take<int32_t>(1);
  HIPCHK(c, hipMemsetAsync(dinfo, 0, 256 * 6, c->stream));
  const float* S = (const float*)b->col[CRUX_COL_S]; const float* w = use_weight ? (const float*)b->col[CRUX_COL_WEIGHT] : nullptr;
  rc = conv_forward_ws(who, v, trunk, S, B); if (rc) return rc;
  const float* feats = conv_act(v, v->L);
  rc = crux_dense_forward(head, feats, B, c->stream); if (rc) return rc;
  crux_launch<TdHeadOp>(1, 256, c->stream, (const float*)crux_dense_act(head, head->nd.L), (const uint8_t*)b->col[CRUX_COL_A], nout, d_y, w, B, dy, st, d_err);
  rc = crux_dense_backward(head, feats, B, dy, 1.0f, true, dfeat, c->stream); if (rc) return rc;
  rc = conv_backward_ws(who, v, trunk, S, B, dfeat, 1.0f, true, nullptr); if (rc) return rc;
  // norm(grads) sees all of Flux.params: one norm over the trunk's and the head's gradient, one gate for both updates
  crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, trunk->g, (int64_t)trunk->nd.n_params, head->g, (int64_t)head->nd.n_params, ssq, Sumsq2Fix{});
  crux_launch<TdInfoOp>(1, 1, c->stream, (const double*)st, (const double*)ssq, B, dinfo);
  rc = adam_gated(trunk, ssq, status); if (rc) return rc;
  rc = adam_gated(head, ssq, status); if (rc) return rc;
  if (!info_out) return crux_launch_check(c, who);      // enqueued only: no synchronisation (a NaN norm still leaves both handles untouched, it is just not reported)
  return finish_step(c, dinfo, status, info_out, who);
}

extern "C" {

int32_t crux_conv_create(crux_ctx* ctx, int32_t W, int32_t H, int32_t C, float in_scale, int32_t n_layers, const crux_conv_layer* layers, crux_conv** out) {
  if (!ctx || !layers || !out) return CRUX_EINVAL;
  if (n_layers < 1 || n_layers > CRUX_CONV_MAXL) return crux_fail(ctx, CRUX_EINVAL, "crux_conv_create: %d layers, 1..%d supported", n_layers, CRUX_CONV_MAXL);
  if (W < 1 || H < 1 || C < 1 || !(in_scale == in_scale)) return crux_fail(ctx, CRUX_EINVAL, "crux_conv_create: input extent %d x %d x %d", W, H, C);
  for (int l = 0; l < n_layers; ++l) {
    if (layers[l].dilation1 != 1 || layers[l].dilation2 != 1) return crux_fail(ctx, CRUX_EUNSUP, "crux_conv_create: layer %d: dilation (%d, %d) is not supported (dilation 1 only)", l, layers[l].dilation1, layers[l].dilation2);
    if (layers[l].groups != 1) return crux_fail(ctx, CRUX_EUNSUP, "crux_conv_create: layer %d: groups = %d is not supported (groups 1 only)", l, layers[l].groups);
  }
  crux_conv* v = new crux_conv(); v->ctx = ctx; v->L = n_layers; v->W = W; v->H = H; v->C = C; v->scale = in_scale;
  int iw = W, ih = H, ic = C; int64_t off = 0;
  v->in_features = (int64_t)W * H * C; v->feat[0] = v->in_features; v->maxfeat = v->in_features;
  for (int l = 0; l < n_layers; ++l) {
    const crux_conv_layer& s = layers[l]; ConvLayerDesc& d = v->ly[l];
    const bool ok = s.k1 >= 1 && s.k2 >= 1 && s.cout >= 1 && s.cin == ic && s.stride1 >= 1 && s.stride2 >= 1 && s.pad1 >= 0 && s.pad2 >= 0 && s.pad1 < s.k1 && s.pad2 < s.k2 &&
                    s.k1 <= iw + 2 * s.pad1 && s.k2 <= ih + 2 * s.pad2 && s.act >= CRUX_ACT_IDENTITY && s.act <= CRUX_ACT_TANH;
    if (!ok) { delete v; return crux_fail(ctx, CRUX_EINVAL, "crux_conv_create: layer %d: Conv((%d, %d), %d => %d, stride (%d, %d), pad (%d, %d), act %d) does not fit its %d x %d x %d input", l, s.k1, s.k2, s.cin, s.cout, s.stride1, s.stride2, s.pad1, s.pad2, s.act, iw, ih, ic); }
    d.k1 = s.k1; d.k2 = s.k2; d.cin = s.cin; d.cout = s.cout; d.s1 = s.stride1; d.s2 = s.stride2; d.p1 = s.pad1; d.p2 = s.pad2; d.act = s.act; d.IW = iw; d.IH = ih;
    d.OW = (iw + 2 * s.pad1 - s.k1) / s.stride1 + 1; d.OH = (ih + 2 * s.pad2 - s.k2) / s.stride2 + 1;
    const int64_t K = (int64_t)s.k1 * s.k2 * s.cin, feat = (int64_t)d.OW * d.OH * s.cout;
    off += K * s.cout + s.cout;
    if (K > (1 << 20) || feat > (1 << 26) || off > 0x7fffffffll) { delete v; return crux_fail(ctx, CRUX_EINVAL, "crux_conv_create: layer %d is too large", l); }
    d.K = (int32_t)K; d.boff = (int32_t)(off - s.cout); d.woff = (int32_t)(d.boff - K * s.cout);
    v->feat[l + 1] = feat; if (feat > v->maxfeat) v->maxfeat = feat;
    iw = d.OW; ih = d.OH; ic = s.cout;
  }
  v->n_params = off;
  *out = v; return CRUX_OK;
}
int32_t crux_conv_destroy(crux_conv* v) {
  if (!v) return CRUX_OK;
  if (v->ws) { crux_sync_before_free(v->ctx); (void)hipFree(v->ws); }
  delete v; return CRUX_OK;
}
int64_t crux_conv_n_params(const crux_conv* v) { return v ? v->n_params : 0; }
int64_t crux_conv_out_features(const crux_conv* v) { return v ? v->feat[v->L] : 0; }
int32_t crux_conv_init_glorot(crux_conv* v, crux_mlp* params, uint64_t seed, uint32_t stream) {
  int32_t rc = conv_check("crux_conv_init_glorot", v, params, 1); if (rc) return rc;
  ConvInit t{}; t.L = v->L; t.n_params = v->n_params;
  for (int l = 0; l < v->L; ++l) { const ConvLayerDesc& d = v->ly[l]; t.woff[l] = d.woff; t.boff[l] = d.boff; t.fan[l] = d.k1 * d.k2 * (d.cin + d.cout); }
  hipLaunchKernelGGL(k_conv_glorot, dim3((unsigned)((v->n_params + 255) / 256)), dim3(256), 0, v->ctx->stream, t, params->p, seed, stream);
  return crux_launch_check(v->ctx, "k_conv_glorot");
}
static int32_t conv_copy_out(crux_conv* v, int64_t B, float* d_y) {
  if (d_y) HIPCHK(v->ctx, hipMemcpyAsync(d_y, conv_act(v, v->L), sizeof(float) * (size_t)v->feat[v->L] * (size_t)B, hipMemcpyDeviceToDevice, v->ctx->stream));
  return CRUX_OK;
}
int32_t crux_conv_forward_cached(crux_conv* v, crux_mlp* params, const float* d_x, int64_t B, float* d_y) {
  if (!d_x) return CRUX_EINVAL;
  int32_t rc = conv_forward_ws("crux_conv_forward", v, params, d_x, B); if (rc) return rc;
  return conv_copy_out(v, B, d_y);
}
int32_t crux_conv_forward(crux_conv* v, crux_mlp* params, const float* d_x, int64_t B, float* d_y) {      // the same pass; the output is not optional
  return d_y ? crux_conv_forward_cached(v, params, d_x, B, d_y) : CRUX_EINVAL;
}
int32_t crux_conv_backward(crux_conv* v, crux_mlp* params, const float* d_x, int64_t B, const float* d_dy, float grad_scale, int32_t want_param_grads, float* d_dx) {
  if (!d_x || !d_dy) return CRUX_EINVAL;
  return conv_backward_ws("crux_conv_backward", v, params, d_x, B, d_dy, grad_scale, want_param_grads != 0, d_dx);
}

int32_t crux_conv_dqn_target(crux_conv* v, crux_mlp* trunk_target, crux_mlp* head_target, crux_buffer* b, float gamma, float* d_y) { CRUX_NO_SN("crux_conv_dqn_target", head_target);      // the head may be wide (crux_mlp_create_wide)
  if (!d_y) return CRUX_EINVAL;
  int32_t rc = conv_pair_check("crux_conv_dqn_target", v, trunk_target, head_target, b); if (rc) return rc;
  crux_ctx* c = v->ctx; const int64_t B = b->elements;
  rc = conv_forward_ws("crux_conv_dqn_target", v, trunk_target, (const float*)b->col[CRUX_COL_SP], B); if (rc) return rc;
  rc = crux_dense_forward(head_target, conv_act(v, v->L), B, c->stream); if (rc) return rc;
  crux_launch<DqnTargetOp>((unsigned)((B + 255) / 256), 256, c->stream, (const float*)crux_dense_act(head_target, head_target->nd.L), (int)head_target->nd.dims[head_target->nd.L],
                           (const float*)b->col[CRUX_COL_R], (const uint8_t*)b->col[CRUX_COL_DONE], gamma, B, d_y);
  return crux_launch_check(c, "crux_conv_dqn_target");
}
int32_t crux_conv_td_step(crux_conv* v, crux_mlp* trunk, crux_mlp* head, crux_buffer* b, const float* d_y, int32_t use_weight, float* info_out) { CRUX_NO_SN("crux_conv_td_step", head);
  return conv_td_step_impl("crux_conv_td_step", v, trunk, head, b, d_y, use_weight, info_out, nullptr);
}
int32_t crux_conv_td_step_with_error(crux_conv* v, crux_mlp* trunk, crux_mlp* head, crux_buffer* b, const float* d_y, int32_t use_weight, float* d_err, float* info_out) { CRUX_NO_SN("crux_conv_td_step_with_error", head);
  if (!d_err) return CRUX_EINVAL;
  return conv_td_step_impl("crux_conv_td_step_with_error", v, trunk, head, b, d_y, use_weight, info_out, d_err);
}

}  // extern "C"
