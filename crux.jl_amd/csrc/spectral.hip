// spectral.hip -- DenseSN (src/extras/spectral_normalization.jl): the power iteration every forward call runs, the effective weights W / sigma the dense engine
// (dense.hip) then reads, and the conversion of the engine's weight gradient G = dL/d(W / sigma) into dL/dW.
//
// Per SN layer with weight W (out x in, column-major W[o + out k]) and the persistent u (out), every forward call does n_iterations times (:2-11)
//   t = W'u, v = t / (|t| + eps);  s = W v, u <- s / (|s| + eps)        eps = eps(Float32) = 2^-23
// then sigma = u'W v (msv, :14) and y = act.((W ./ sigma) x .+ b) (:41). u and v come out of ignore_derivatives (:40), msv is differentiated through W:
//   dL/dW = G / sigma - (<G, W> / sigma^2) u v'      dL/db unchanged
// k_sn_power: ONE launch per forward pass, one workgroup of 256 per SN layer. Both passes over W are coalesced: W'u gives each wave a column (lanes walk down it, the
// wave adds with the xor butterfly), W v gives each thread a row (neighbouring threads read neighbouring rows of one column); layers with fewer than 256 rows split the
// columns over 256 / rows' thread groups whose partial sums are added in group order. u, v and s stay in LDS (dims <= 1024), W is read from L2 2 n_iterations + 1 times.
// With the final u, sigma = u's (s = W v of the last iteration): no further pass. Every sum has a fixed order, there are no float atomics: two identical calls give
// identical bits. k_sn_grad: one workgroup per SN layer, <G, W> in Float64 (thread-strided, wave butterfly, waves in order), then the in-place rewrite of the layer's
// slice of the gradient with the u, v and sigma the matching forward pass left.
#include "common.h"

#define SN_EPS 1.1920928955078125e-07f

__device__ __forceinline__ float sn_block_sum(float v, float* red) {      // wave butterfly, then the four wave sums in wave order
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_sn_power(const crux_sn_layer* __restrict__ tab, const float* __restrict__ p, float* __restrict__ weff, float* __restrict__ u, float* __restrict__ v,
                                                  float* __restrict__ sigma) {
  __shared__ float su[1024], sv[1024], ss[1024], spart[256], red[4];
  const crux_sn_layer L = tab[blockIdx.x];
  const int in = L.in, out = L.out, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* __restrict__ W = p + L.woff;
  for (int o = tid; o < out; o += 256) su[o] = u[L.uoff + o];
  // rows' = the power of two >= out (at most 256); the 256 / rows' groups take ceil(in / groups) columns each in the W v pass
  int rp = 1; while (rp < out && rp < 256) rp <<= 1;
  const int ngrp = 256 / rp, kc = (in + ngrp - 1) / ngrp, r = tid & (rp - 1), grp = tid / rp;
  float sg = 0.f;
  __syncthreads();
  for (int it = 0; it < L.iters; ++it) {
    for (int k = wv; k < in; k += 4) {                                   // t = W'u: a column per wave
      const float* col = W + (int64_t)out * k; float a = 0.f;
      for (int o = lane; o < out; o += 64) a = fmaf(col[o], su[o], a);
      a = wave_sum(a);
      if (lane == 0) sv[k] = a;
    }
    __syncthreads();
    float q = 0.f; for (int k = tid; k < in; k += 256) q = fmaf(sv[k], sv[k], q);
    const float nt = sqrtf(sn_block_sum(q, red)) + SN_EPS;
    for (int k = tid; k < in; k += 256) sv[k] = sv[k] / nt;              // v
    __syncthreads();
    for (int o0 = 0; o0 < out; o0 += rp) {                               // s = W v: a row per thread (ngrp > 1: out <= rp, one round)
      const int o = o0 + r; float a = 0.f;
      if (o < out) { const int k1 = (grp + 1) * kc < in ? (grp + 1) * kc : in; for (int k = grp * kc; k < k1; ++k) a = fmaf(W[o + (int64_t)out * k], sv[k], a); }
      if (ngrp == 1) { if (o < out) ss[o] = a; } else spart[tid] = a;
    }
    if (ngrp > 1) {
      __syncthreads();
      if (tid < out) { float a = spart[tid]; for (int gq = 1; gq < ngrp; ++gq) a += spart[gq * rp + tid]; ss[tid] = a; }
    }
    __syncthreads();
    q = 0.f; for (int o = tid; o < out; o += 256) q = fmaf(ss[o], ss[o], q);
    const float ns = sqrtf(sn_block_sum(q, red)) + SN_EPS;
    for (int o = tid; o < out; o += 256) su[o] = ss[o] / ns;             // u
    __syncthreads();
    if (it == L.iters - 1) { q = 0.f; for (int o = tid; o < out; o += 256) q = fmaf(su[o], ss[o], q); sg = sn_block_sum(q, red); }      // sigma = u'(W v)
  }
  for (int o = tid; o < out; o += 256) u[L.uoff + o] = su[o];
  for (int k = tid; k < in; k += 256) v[L.voff + k] = sv[k];
  if (tid == 0) sigma[L.idx] = sg;
  float* __restrict__ E = weff + L.woff; const int n = in * out;
  for (int i = tid; i < n; i += 256) E[i] = W[i] / sg;                   // W ./ sigma (:41)
}

__global__ __launch_bounds__(256) void k_sn_grad(const crux_sn_layer* __restrict__ tab, const float* __restrict__ p, float* __restrict__ g, const float* __restrict__ u, const float* __restrict__ v,
                                                 const float* __restrict__ sigma) {
  __shared__ double red[4];
  const crux_sn_layer L = tab[blockIdx.x];
  const int out = L.out, n = L.in * L.out, tid = threadIdx.x;
  const float* __restrict__ W = p + L.woff; float* __restrict__ G = g + L.woff;
  double a = 0; for (int i = tid; i < n; i += 256) a += (double)G[i] * (double)W[i];
  a = wave_sum_d(a);
  if ((tid & 63) == 0) red[tid >> 6] = a;
  __syncthreads();
  const double dot = ((red[0] + red[1]) + red[2]) + red[3];
  const float sg = sigma[L.idx], cf = (float)(dot / ((double)sg * (double)sg));
  const float* uu = u + L.uoff; const float* vv = v + L.voff;
  for (int i = tid; i < n; i += 256) { const int k = i / out, o = i - k * out; G[i] = G[i] / sg - cf * uu[o] * vv[k]; }
}

int32_t crux_sn_power(crux_mlp* n, hipStream_t st) {
  const crux_sn* s = n->sn;
  hipLaunchKernelGGL(k_sn_power, dim3((unsigned)s->n_sn), dim3(256), 0, st, (const crux_sn_layer*)s->tab, (const float*)n->p, s->weff, s->u, s->v, s->sigma);
  return crux_launch_check(n->ctx, "k_sn_power");
}
int32_t crux_sn_grad(crux_mlp* n, hipStream_t st) {
  const crux_sn* s = n->sn;
  hipLaunchKernelGGL(k_sn_grad, dim3((unsigned)s->n_sn), dim3(256), 0, st, (const crux_sn_layer*)s->tab, (const float*)n->p, n->g, (const float*)s->u, (const float*)s->v, (const float*)s->sigma);
  return crux_launch_check(n->ctx, "k_sn_grad");
}
void crux_sn_free(crux_mlp* n) {      // the caller has synchronised the stream
  if (!n->sn) return;
  (void)hipFree(n->sn->block); delete n->sn; n->sn = nullptr;
}
int32_t crux_plain_only(const char* entry, std::initializer_list<const crux_mlp*> nets) {
  for (const crux_mlp* q : nets) if (q && q->sn)
    return crux_fail(q->ctx, CRUX_EUNSUP, "%s: a handle with spectrally normalised layers (crux_mlp_set_spectral) was passed; this entry reads the raw weights and would ignore the normalisation", entry);
  return CRUX_OK;
}
int32_t crux_narrow_only(const char* entry, std::initializer_list<const crux_mlp*> nets) {
  for (const crux_mlp* q : nets) if (q && q->wide)
    return crux_fail(q->ctx, CRUX_EUNSUP, "%s: a wide handle (crux_mlp_create_wide, widest layer %d > 1024) was passed; this entry is outside the dense engine's passes that take one", entry, q->nd.maxdim);
  return CRUX_OK;
}
int32_t crux_no_clip(const char* entry, std::initializer_list<const crux_mlp*> nets) {
  for (const crux_mlp* q : nets) if (q && q->clip > 0.f)
    return crux_fail(q->ctx, CRUX_EUNSUP, "%s: a handle with ClipValue(%g) in front of Adam (crux_adam_set_clip_value) was passed; this update would ignore the clamp", entry, (double)q->clip);
  return CRUX_OK;
}

extern "C" {

int32_t crux_mlp_set_spectral(crux_mlp* n, const int32_t* n_iter, const float* host_u, uint64_t seed, uint32_t stream) {
  if (!n || !n_iter) return CRUX_EINVAL;
  CRUX_NARROW_ONLY("crux_mlp_set_spectral", n);
  crux_ctx* c = n->ctx; const NetDesc& nd = n->nd;
  if (nd.L < 1) return crux_fail(c, CRUX_EINVAL, "set_spectral: the handle has no layers");
  int n_sn = 0, n_u = 0, n_v = 0;
  for (int l = 0; l < nd.L; ++l) {
    if (n_iter[l] < 0 || n_iter[l] > 8) return crux_fail(c, CRUX_EINVAL, "set_spectral: n_iterations of layer %d = %d, must be 0 (plain Dense) or 1..8", l, n_iter[l]);
    if (n_iter[l]) { ++n_sn; n_u += nd.dims[l + 1]; n_v += nd.dims[l]; }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  crux_sn_free(n);
  if (!n_sn) return CRUX_OK;      // all plain: the handle is a plain Chain(Dense...) again
  crux_sn* s = new crux_sn();
  crux_sn_layer tab[CRUX_MAXL]; int q = 0, uo = 0, vo = 0;
  for (int l = 0; l < nd.L; ++l) {
    s->iters[l] = n_iter[l];
    if (!n_iter[l]) continue;
    tab[q] = crux_sn_layer{nd.dims[l], nd.dims[l + 1], nd.woff[l], uo, vo, n_iter[l], q, 0};
    uo += nd.dims[l + 1]; vo += nd.dims[l]; ++q;
  }
  s->n_sn = n_sn; s->n_u = n_u; s->n_v = n_v;
  const size_t bw = Carve::span<float>((size_t)nd.xoff), bu = Carve::span<float>((size_t)n_u), bv = Carve::span<float>((size_t)n_v), bs = Carve::span<float>((size_t)n_sn),
               bt = Carve::span<crux_sn_layer>((size_t)n_sn);
  if (hipMalloc(&s->block, bw + bu + bv + bs + bt) != hipSuccess) { delete s; return crux_fail(c, CRUX_ENOMEM, "set_spectral: hipMalloc(%zu) failed", bw + bu + bv + bs + bt); }
  Carve cv{(char*)s->block, 0};
  s->weff = cv.take<float>((size_t)nd.xoff); s->u = cv.take<float>((size_t)n_u); s->v = cv.take<float>((size_t)n_v); s->sigma = cv.take<float>((size_t)n_sn); s->tab = cv.take<crux_sn_layer>((size_t)n_sn);
  n->sn = s;
  std::vector<float> hu((size_t)n_u);
  if (host_u) memcpy(hu.data(), host_u, sizeof(float) * (size_t)n_u);
  else for (int i = 0; i < n_u; ++i) {      // randn(Float32, out, 1) (:31): Box-Muller's first output of Philox(seed, i, stream, NOISE), the library's standard normal
    const crux_u32x4 x = crux_philox(seed, (uint64_t)i, stream, CRUX_RNG_NOISE);
    const double u1 = crux_u32x2_to_f64(x.v[0], x.v[1]), u2 = crux_u32x2_to_f64(x.v[2], x.v[3]);
    hu[(size_t)i] = (float)(sqrt(-2.0 * log(1.0 - u1)) * cos(2.0 * M_PI * u2));
  }
  HIPCHK(c, hipMemsetAsync(s->block, 0, bw + bu + bv + bs, c->stream));
  HIPCHK(c, hipMemcpyAsync(s->u, hu.data(), sizeof(float) * (size_t)n_u, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(s->tab, tab, sizeof(crux_sn_layer) * (size_t)n_sn, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // hu and tab are host temporaries
  return CRUX_OK;
}

int32_t crux_mlp_get_spectral(crux_mlp* n, float* host_u, float* host_v, float* host_sigma) {
  if (!n) return CRUX_EINVAL;
  crux_ctx* c = n->ctx; const crux_sn* s = n->sn;
  if (!s) return crux_fail(c, CRUX_EINVAL, "get_spectral: the handle has no spectrally normalised layer");
  if (host_u) HIPCHK(c, hipMemcpyAsync(host_u, s->u, sizeof(float) * (size_t)s->n_u, hipMemcpyDeviceToHost, c->stream));
  if (host_v) HIPCHK(c, hipMemcpyAsync(host_v, s->v, sizeof(float) * (size_t)s->n_v, hipMemcpyDeviceToHost, c->stream));
  if (host_sigma) HIPCHK(c, hipMemcpyAsync(host_sigma, s->sigma, sizeof(float) * (size_t)s->n_sn, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CRUX_OK;
}

int32_t crux_mlp_spectral_layers(const crux_mlp* n, int32_t* n_iter) {
  if (!n) return CRUX_EINVAL;
  for (int l = 0; l < n->nd.L && n_iter; ++l) n_iter[l] = n->sn ? n->sn->iters[l] : 0;
  return n->sn ? n->sn->n_sn : 0;
}

}  // extern "C"
