// iq.hip -- off-policy imitation learning: the gradient penalty (src/extras/gradient_penalty.jl) and the critic step of OnlineIQLearn (iq_loss,
// src/model_free/il/iqlearn.jl:49-95) on the dense engine (dense.hip). Reference of the update: train! src/training.jl:13-25 (gradient norm, NaN => error
// before the update, Adam).
//
// Notation: z_l = W_l h_{l-1} + b_l, h_l = s_l(z_l), l = 1..L. Activations are identity, relu or tanh; their derivatives are formed from h:
// s'_relu = [h > 0], s'_tanh = 1 - h^2, s''_tanh = -2 h (1 - h^2), s''_relu = s''_identity = 0.
//
// One call over a staging minibatch of B columns (B_p policy rows first, then the demo rows) and H = B_e penalty columns:
//   k_iq_expand     X = [s | s' | xhat], xhat_j = eps_j xtilde_j + (1 - eps_j) x_j (x = the demo state, xtilde = the policy state); NaN anywhere -> nanflag
//   dense forward   Q over all 2B + H columns, activations cached
//   k_iq_head       V = logsumexp Q(s), V' = logsumexp Q(s'), y = gamma_iq (1 - done) V', R = Q(s, a) - y; seeds of the s and s' columns; fixed-order sums
//   data gradient   dZ_l and G_{l-1} = W_l^T dZ_l over all columns (the xhat columns are seeded with ones: their dZ_l is delta_l, their G_l is g_l)
//   weight gradient of the loss over the first 2B columns only: the ones seed of the xhat columns never enters it
//   k_iq_gp_head    |g_0| per xhat column, P = mean (|g_0| - target)^2, seed gbar_0 = lambda 2 (|g_0| - target) g_0 / |g_0| / H
//   upward sweep    l = 1..L: T1_l = delta_l gbar_{l-1}^T, dbar_l = W_l gbar_{l-1}, gbar_l = s'_l dbar_l, z2_l = dbar_l g_l s''_l (g_L = 1)
//   downward sweep  (only when a layer is tanh; z2 = 0 otherwise) zbar_l = z2_l + s'_l W_{l+1}^T zbar_{l+1}; T2_l = zbar_l h_{l-1}^T, db_l = sum zbar_l
//   k_iq_addgrad    g += T1 + T2 (one fixed-order add), then the norm, the info row, the NaN gate and Adam as every *_step
// Every product is a Gemm16 launch (dense.hip); no float atomics anywhere, so two identical calls give identical bits.
// |g_0| = 0 gives a NaN seed (0 / 0), as Zygote's pullback of sqrt at 0 does (Inf * 0): the step then stops with "NaN detected!".
// Randomness: eps_j = (float)u53(Philox(seed, counter, j, IQ_GP)) (include/crux_rng.h).
#include "common.h"
#include "exec.h"

// ---- the column matrix X = [s (nl) | s' (nl) | xhat (H)] -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_iq_expand(const float* __restrict__ s, const float* __restrict__ sp, int64_t nl, const float* __restrict__ x, const float* __restrict__ xt,
                                                   int64_t H, int od, uint64_t seed, uint64_t counter, float* __restrict__ X, int32_t* __restrict__ nanflag) {
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (col >= 2 * nl + H) return;
  float* o = X + col * od; bool bad = false;
  if (col < nl) { for (int k = 0; k < od; ++k) { const float v = s[col * od + k]; o[k] = v; bad = bad || v != v; } }
  else if (col < 2 * nl) { const int64_t j = col - nl; for (int k = 0; k < od; ++k) { const float v = sp[j * od + k]; o[k] = v; bad = bad || v != v; } }
  else {
    const int64_t j = col - 2 * nl;
    if (xt) {
      const crux_u32x4 r = crux_philox(seed, counter, (uint32_t)j, CRUX_RNG_IQ_GP); const float e = (float)crux_u32x2_to_f64(r.v[0], r.v[1]);
      const float ce = __fsub_rn(1.f, e);
      for (int k = 0; k < od; ++k) { const float a = x[j * od + k], b = xt[j * od + k]; const float v = __fadd_rn(__fmul_rn(e, b), __fmul_rn(ce, a));
        o[k] = v; bad = bad || a != a || b != b; }
    } else { for (int k = 0; k < od; ++k) { const float v = x[j * od + k]; o[k] = v; bad = bad || v != v; } }
  }
  // the engine's relu maps NaN to 0, where NNlib's propagates it: the heads are told instead and poison what they form
  if (bad) atomicOr((int*)nanflag, 1);
}

// ---- iq_loss head (one block of 256, fixed order) -------------------------------------------------------------------------------------------------------------------
// Q: [A x (2B + ...)] network outputs; columns [0, B) are Q(s), [B, 2B) Q(s'). Rows b >= Bp are the demo (expert) rows.
// stats: [0] sum_E (-R), [1] sum (V - y), [2] sum_{policy} R, [3] sum R^2
__global__ __launch_bounds__(256) void k_iq_head(const float* __restrict__ Q, const uint8_t* __restrict__ a, const uint8_t* __restrict__ done, int A, int64_t B, int64_t Bp,
                                                 float gamma, int reg, float alpha_reg, const int32_t* __restrict__ nanflag, float* __restrict__ dy, double* __restrict__ stats) {
  __shared__ double red[4];
  const bool poison = nanflag[0] != 0; const float invB = 1.f / (float)B, invBe = 1.f / (float)(B - Bp), rs = reg ? 1.f / (2.f * alpha_reg * (float)B) : 0.f;
  double s_e = 0, s_v = 0, s_p = 0, s_r2 = 0;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    const float* q = Q + b * A; const float* qp = Q + (B + b) * A; const uint8_t* ab = a + b * A;
    float m = -INFINITY, mp = -INFINITY, qa = 0.f;
    for (int k = 0; k < A; ++k) { m = fmaxf(m, q[k]); mp = fmaxf(mp, qp[k]); qa += q[k] * (ab[k] ? 1.f : 0.f); }
    float se = 0.f, sep = 0.f;
    for (int k = 0; k < A; ++k) { se += expf(q[k] - m); sep += expf(qp[k] - mp); }
    const float V = m + logf(se), Vp = mp + logf(sep);
    const float gd = gamma * (1.f - (done[b] ? 1.f : 0.f));
    const float y = gd * Vp; const float R = qa - y;
    const bool ex = b >= Bp;
    const float dR = (ex ? -invBe : 0.f) + R * rs;
    const float cp = (-dR - invB) * gd;
    float* d = dy + b * A; float* dp = dy + (B + b) * A;
    for (int k = 0; k < A; ++k) {
      const float g = dR * (ab[k] ? 1.f : 0.f) + (expf(q[k] - m) / se) * invB, gp = cp * (expf(qp[k] - mp) / sep);
      d[k] = poison ? NAN : g; dp[k] = poison ? NAN : gp;
    }
    if (ex) s_e += (double)(-R); else s_p += (double)R;
    s_v += (double)(V - y); s_r2 += (double)(R * R);
  }
  s_e = block_sum256(s_e, red); s_v = block_sum256(s_v, red); s_p = block_sum256(s_p, red); s_r2 = block_sum256(s_r2, red);
  if (threadIdx.x == 0) { const double pz = poison ? NAN : 0.0; stats[0] = s_e + pz; stats[1] = s_v + pz; stats[2] = s_p + pz; stats[3] = s_r2 + pz; }
}

// ---- gradient-penalty head (one block of 256, fixed order): g0 [od x H] input gradients of the xhat columns --------------------------------------------------------
// stats[4] = sum_j (|g_j| - target)^2; gbar [od x H] = lambda 2 (|g_j| - target) / H * g_j / |g_j| (NULL: value only)
__global__ __launch_bounds__(256) void k_iq_gp_head(const float* __restrict__ g0, int od, int64_t H, float target, float lambda, const int32_t* __restrict__ nanflag,
                                                    float* __restrict__ gbar, double* __restrict__ stats) {
  __shared__ double red[4];
  const bool poison = nanflag[0] != 0; const float cs = 2.f * lambda / (float)H;
  double s = 0;
  for (int64_t j = threadIdx.x; j < H; j += 256) {
    const float* g = g0 + j * od; float ss = 0.f;
    for (int k = 0; k < od; ++k) ss += g[k] * g[k];
    const float n = sqrtf(ss), dv = n - target;
    s += (double)(dv * dv);
    if (gbar) { const float c = cs * dv; for (int k = 0; k < od; ++k) gbar[j * od + k] = poison ? NAN : c * (g[k] / n); }
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) stats[4] = poison ? NAN : s;
}

// ---- element-wise pieces of the sweeps ------------------------------------------------------------------------------------------------------------------------------
// tangent: gbar_l = s'_l(h) dbar (gnext may be NULL: the output layer), z2 = dbar g s''_l(h) (g NULL: g_L = 1; z2 NULL: no second-order sweep)
__global__ __launch_bounds__(256) void k_iq_tangent(const float* __restrict__ dbar, const float* __restrict__ h, const float* __restrict__ g, int act, int64_t n,
                                                    float* __restrict__ gnext, float* __restrict__ z2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
  const float d = dbar[i], y = h[i];
  if (gnext) gnext[i] = crux_act_grad(act, y, d);
  if (z2) { const float gg = g ? g[i] : 1.f; z2[i] = act == CRUX_ACT_TANH ? d * gg * (-2.f * y * (1.f - y * y)) : 0.f; }
}
// injection of the downward sweep: z[i] (holding z2_l) += s'_l(h) hb
__global__ __launch_bounds__(256) void k_iq_inject(const float* __restrict__ hb, const float* __restrict__ h, int act, int64_t n, float* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
  z[i] = z[i] + crux_act_grad(act, h[i], hb[i]);
}
// g = g + (T1 + T2): the penalty's share added to the gradient already there (the loss's, or whatever the caller accumulated)
__global__ __launch_bounds__(256) void k_iq_addgrad(float* __restrict__ g, const float* __restrict__ t1, const float* __restrict__ t2, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
  g[i] = g[i] + (t1[i] + t2[i]);
}
// info row LOSS, GRAD_NORM and the six iq_loss values: softQloss, valueloss, avg_R_expert_IQ, avg_R_demo_IQ, grad_pen, reg_loss
__global__ void k_iq_info(const double* __restrict__ st, const double* __restrict__ ssq, int64_t B, int64_t Bp, int64_t H, int gp, float lambda_gp, int reg, float alpha_reg,
                          float* __restrict__ dinfo, float* __restrict__ iq) {
  if (threadIdx.x != 0) return;
  ssq_finalize(ssq);
  const float p1 = (float)(st[0] / (double)(B - Bp)), p2 = (float)(st[1] / (double)B);
  const float gpv = gp ? lambda_gp * (float)(st[4] / (double)H) : 0.f;
  const float rl = reg ? (1.f / (4.f * alpha_reg)) * (float)(st[3] / (double)B) : 0.f;
  float loss = p1 + p2; if (gp) loss = loss + gpv; if (reg) loss = loss + rl;
  dinfo[CRUX_INFO_LOSS] = loss; dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(ssq[0]);
  iq[0] = p1; iq[1] = p2; iq[2] = -p1; iq[3] = (float)(st[2] / (double)Bp); iq[4] = gpv; iq[5] = rl;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------------
struct IqBufs : StepSmall {      // extra: the six iq_loss values (advil.hip: the step's four)
  float* X; float* dy; float* Z[CRUX_MAXL + 1]; float* G[CRUX_MAXL + 1]; float* gb[2]; float* dbar; float* t1; float* t2;
  float* own;      // own_floats of the caller's behind everything else (advil.hip: expert_sa and pi_sa)
};
static bool iq_has_tanh(const NetDesc& nd) { for (int l = 0; l < nd.L; ++l) if (nd.acts[l] == CRUX_ACT_TANH) return true; return false; }
static int32_t iq_check_net(crux_ctx* c, const crux_mlp* n, const char* who) {
  const NetDesc& nd = n->nd;
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  if (nd.L < 1) return crux_fail(c, CRUX_EINVAL, "%s: the handle has no layers", who);
  for (int l = 0; l < nd.L; ++l) if (nd.acts[l] != CRUX_ACT_IDENTITY && nd.acts[l] != CRUX_ACT_RELU && nd.acts[l] != CRUX_ACT_TANH)
    return crux_fail(c, CRUX_EUNSUP, "%s: activation %d of layer %d", who, nd.acts[l], l + 1);
  return CRUX_OK;
}
// scratch for nl loss columns (0 or B) and H penalty columns; second-order buffers only when want_pg; own_floats: a piece for the caller in the same block
static int32_t iq_prepare(crux_mlp* n, int64_t nl, int64_t H, bool want_pg, IqBufs& ib, const char* who, size_t own_floats = 0) {
  crux_ctx* c = n->ctx; const NetDesc& nd = n->nd; const int64_t NC = 2 * nl + H; const size_t np = (size_t)nd.n_params;
  size_t fl = (size_t)nd.dims[0] * NC + (size_t)nd.dims[nd.L] * NC;
  for (int l = 1; l <= nd.L; ++l) fl += (size_t)nd.dims[l] * NC;        // Z_l
  for (int l = 0; l < nd.L; ++l) fl += (size_t)nd.dims[l] * NC;         // G_l
  if (want_pg) fl += 3 * (size_t)nd.maxdim * H + 2 * np;
  const size_t bytes = 4 * fl + 256 * (2 * CRUX_MAXL + 10) + STEP_SMALL + (own_floats ? Carve::span<float>(own_floats) : 0);
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  ib.X = cv.take<float>((size_t)nd.dims[0] * NC); ib.dy = cv.take<float>((size_t)nd.dims[nd.L] * NC);
  for (int l = 1; l <= nd.L; ++l) ib.Z[l] = cv.take<float>((size_t)nd.dims[l] * NC);
  for (int l = 0; l < nd.L; ++l) ib.G[l] = cv.take<float>((size_t)nd.dims[l] * NC);
  if (want_pg) { ib.gb[0] = cv.take<float>((size_t)nd.maxdim * H); ib.gb[1] = cv.take<float>((size_t)nd.maxdim * H); ib.dbar = cv.take<float>((size_t)nd.maxdim * H);
                 ib.t1 = cv.take<float>(np); ib.t2 = cv.take<float>(np); }
  { const int32_t rc = step_small(c, cv, ib); if (rc) return rc; }
  ib.own = own_floats ? cv.take<float>(own_floats) : nullptr;
  if (want_pg) HIPCHK(c, hipMemsetAsync(ib.t1, 0, 4 * np, c->stream));       // T1's bias entries stay zero; t2 is zeroed below when there is no second-order sweep
  if (want_pg) HIPCHK(c, hipMemsetAsync(ib.t2, 0, 4 * np, c->stream));
  return CRUX_OK;
}
// C[i, j] = sum_k A(i, k) B(k, j) with no epilogue (EPI_BWD_DATA without an activation source)
static int32_t iq_gemm(crux_ctx* c, const float* A, int64_t sAi, int64_t sAk, const float* Bm, int64_t sBk, int64_t sBj, int M, int N, int K, float* Cm, int64_t sCj) {
  GemmArgs q{}; q.A = A; q.sAi = sAi; q.sAk = sAk; q.B = Bm; q.sBk = sBk; q.sBj = sBj; q.M = M; q.N = N; q.K = K; q.C = Cm; q.sCj = sCj; q.epi = EPI_BWD_DATA;
  q.ysrc = nullptr; q.act = CRUX_ACT_IDENTITY;
  return launch_gemm(c, q, c->stream);
}
// dW[o, k] = scale sum_j dZ[o, j] X[k, j] over K columns (db[o] = scale sum_j dZ[o, j] when db != NULL)
static int32_t iq_wgrad(crux_ctx* c, const float* dZ, const float* X, int out, int in, int64_t K, float* dW, float* db, float scale = 1.0f) {
  GemmArgs q{}; q.A = dZ; q.sAi = 1; q.sAk = out; q.B = X; q.sBk = in; q.sBj = 1; q.M = out; q.N = in; q.K = (int)K;
  q.C = dW; q.sCj = out; q.epi = EPI_WGRAD; q.scale = scale; q.gbias = db; q.nf = nullptr;
  return launch_gemm(c, q, c->stream);
}
// data-gradient pass over all NC columns after the forward pass and the seeds: Z_l = dZ_l, G_l = W_{l+1}^T dZ_{l+1} (G_0 over the H penalty columns only)
static int32_t iq_dgrad(crux_mlp* n, int64_t nl, int64_t H, const IqBufs& ib) {
  crux_ctx* c = n->ctx; const NetDesc& nd = n->nd; const int64_t NC = 2 * nl + H; const int L = nd.L;
  const int64_t cnt = (int64_t)nd.dims[L] * NC;
  crux_launch<ActGradOp>(nblk(cnt), 256, c->stream, (const float*)ib.dy, (const float*)crux_dense_act(n, L), nd.acts[L - 1], cnt, ib.Z[L]);
  int32_t rc = crux_launch_check(c, "k_act_grad"); if (rc) return rc;
  for (int l = L; l >= 1; --l) {
    const int in = nd.dims[l - 1], out = nd.dims[l];
    if (l == 1) {
      if (H == 0) break;
      rc = iq_gemm(c, n->p + nd.woff[0], out, 1, ib.Z[1] + 2 * nl * out, 1, out, in, (int)H, out, ib.G[0] + 2 * nl * in, in); if (rc) return rc;
      break;
    }
    rc = iq_gemm(c, n->p + nd.woff[l - 1], out, 1, ib.Z[l], 1, out, in, (int)NC, out, ib.G[l - 1], in); if (rc) return rc;
    const int64_t m = (int64_t)in * NC;
    crux_launch<ActGradOp>(nblk(m), 256, c->stream, (const float*)ib.G[l - 1], (const float*)crux_dense_act(n, l - 1), nd.acts[l - 2], m, ib.Z[l - 1]);
    rc = crux_launch_check(c, "k_act_grad"); if (rc) return rc;
  }
  return CRUX_OK;
}
// lambda dP/dtheta into ib.t1 + ib.t2 after iq_dgrad and k_iq_gp_head (ib.gb[0] = gbar_0), over the H penalty columns at offset 2 nl
static int32_t iq_penalty_sweeps(crux_mlp* n, int64_t nl, int64_t H, const IqBufs& ib) {
  crux_ctx* c = n->ctx; const NetDesc& nd = n->nd; const int L = nd.L; const int64_t c0 = 2 * nl;
  const bool second = iq_has_tanh(nd); int32_t rc;
  const float* gprev = ib.gb[0]; int cur = 1;
  for (int l = 1; l <= L; ++l) {          // upward tangent sweep
    const int in = nd.dims[l - 1], out = nd.dims[l];
    float* zl = ib.Z[l] + c0 * out;       // delta_l of the penalty columns; overwritten by z2_l below (after T1_l has read it, stream order)
    rc = iq_wgrad(c, zl, gprev, out, in, H, ib.t1 + nd.woff[l - 1], nullptr); if (rc) return rc;
    const bool need_g = l < L, need_z2 = second;
    if (!need_g && !need_z2) break;
    rc = iq_gemm(c, n->p + nd.woff[l - 1], 1, out, gprev, 1, in, out, (int)H, in, ib.dbar, out); if (rc) return rc;
    float* gn = need_g ? ib.gb[cur] : nullptr;
    const int64_t m = (int64_t)out * H;
    hipLaunchKernelGGL(k_iq_tangent, dim3(nblk(m)), dim3(256), 0, c->stream, (const float*)ib.dbar, (const float*)(crux_dense_act(n, l) + c0 * out),
                       (const float*)(l < L ? ib.G[l] + c0 * out : nullptr), nd.acts[l - 1], m, gn, need_z2 ? zl : nullptr);
    rc = crux_launch_check(c, "k_iq_tangent"); if (rc) return rc;
    if (gn) { gprev = gn; cur ^= 1; }
  }
  if (!second) return CRUX_OK;            // relu / identity networks: every z2 is zero and so is the whole downward sweep (t2 stays zero)
  for (int l = L; l >= 1; --l) {          // downward sweep through the forward graph, injecting z2
    const int in = nd.dims[l - 1], out = nd.dims[l];
    const float* zl = ib.Z[l] + c0 * out;
    const float* hx = l == 1 ? ib.X + c0 * in : crux_dense_act(n, l - 1) + c0 * in;
    rc = iq_wgrad(c, zl, hx, out, in, H, ib.t2 + nd.woff[l - 1], ib.t2 + nd.boff[l - 1]); if (rc) return rc;
    if (l == 1) break;
    rc = iq_gemm(c, n->p + nd.woff[l - 1], out, 1, zl, 1, out, in, (int)H, out, ib.dbar, in); if (rc) return rc;
    const int64_t m = (int64_t)in * H;
    hipLaunchKernelGGL(k_iq_inject, dim3(nblk(m)), dim3(256), 0, c->stream, (const float*)ib.dbar, (const float*)(crux_dense_act(n, l - 1) + c0 * in), nd.acts[l - 2], m,
                       ib.Z[l - 1] + c0 * in);
    rc = crux_launch_check(c, "k_iq_inject"); if (rc) return rc;
  }
  return CRUX_OK;
}
static int32_t iq_add_penalty(crux_mlp* n, const IqBufs& ib) {
  crux_ctx* c = n->ctx; const int64_t np = n->nd.n_params;
  hipLaunchKernelGGL(k_iq_addgrad, dim3(nblk(np)), dim3(256), 0, c->stream, n->g, (const float*)ib.t1, (const float*)ib.t2, np);
  return crux_launch_check(c, "k_iq_addgrad");
}

extern "C" {

int32_t crux_gradient_penalty(crux_mlp* net, const float* d_x, const float* d_xtilde, int64_t B, float target, float lambda, int32_t accumulate,
                              uint64_t seed, uint64_t counter, float* penalty_out) { CRUX_PLAIN_ONLY("crux_gradient_penalty", net);
  if (!net || !d_x || !penalty_out) return CRUX_EINVAL;
  crux_ctx* c = net->ctx; const char* who = "gradient_penalty"; const NetDesc& nd = net->nd;
  int32_t rc = iq_check_net(c, net, who); if (rc) return rc;
  if (B < 1 || B > (1 << 20)) return crux_fail(c, CRUX_EINVAL, "%s: batch %lld out of range", who, (long long)B);
  IqBufs ib{}; rc = iq_prepare(net, 0, B, accumulate != 0, ib, who); if (rc) return rc;
  hipLaunchKernelGGL(k_iq_expand, dim3(nblk(B)), dim3(256), 0, c->stream, (const float*)nullptr, (const float*)nullptr, (int64_t)0, d_x, d_xtilde, B, nd.dims[0], seed, counter,
                     ib.X, ib.nanflag);
  rc = crux_launch_check(c, "k_iq_expand"); if (rc) return rc;
  rc = crux_dense_forward(net, ib.X, B, c->stream); if (rc) return rc;
  const int64_t ny = (int64_t)nd.dims[nd.L] * B;
  crux_launch<FillOp>(nblk(ny), 256, c->stream, ib.dy, 1.0f, ny);
  rc = iq_dgrad(net, 0, B, ib); if (rc) return rc;
  hipLaunchKernelGGL(k_iq_gp_head, dim3(1), dim3(256), 0, c->stream, (const float*)ib.G[0], nd.dims[0], B, target, lambda, (const int32_t*)ib.nanflag,
                     accumulate ? ib.gb[0] : nullptr, ib.stats);
  rc = crux_launch_check(c, "k_iq_gp_head"); if (rc) return rc;
  if (accumulate) {
    rc = iq_penalty_sweeps(net, 0, B, ib); if (rc) return rc;
    rc = iq_add_penalty(net, ib); if (rc) return rc;
  }
  double h = 0;
  HIPCHK(c, hipMemcpyAsync(&h, ib.stats + 4, sizeof h, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  *penalty_out = (float)(h / (double)B);
  return CRUX_OK;
}

int32_t crux_iq_step(crux_mlp* q, crux_buffer* b, int64_t n_policy, float gamma_iq, int32_t reg, float alpha_reg, int32_t gp, float lambda_gp,
                     uint64_t seed, uint64_t counter, float* info_out, float* iq_out) { CRUX_PLAIN_ONLY("crux_iq_step", q);
  if (!q || !b) return CRUX_EINVAL;
  crux_ctx* c = q->ctx; const char* who = "iq_loss"; const NetDesc& nd = q->nd;
  int32_t rc = iq_check_net(c, q, who); if (rc) return rc;
  const int64_t B = b->elements, Bp = n_policy, Be = B - n_policy; const int od = b->obs_dim, A = b->act_dim;
  if (b->act_kind != CRUX_ACTION_DISCRETE) return crux_fail(c, CRUX_EINVAL, "%s: needs a DiscreteNetwork (one-hot action column)", who);
  if (nd.dims[0] != od || nd.dims[nd.L] != A || nd.n_extra != 0) return crux_fail(c, CRUX_EINVAL, "%s: Q must map %d -> %d", who, od, A);
  if (B < 2 || B > (1 << 20)) return crux_fail(c, CRUX_EINVAL, "%s: batch %lld out of range", who, (long long)B);
  if (Bp < 1 || Be < 1) return crux_fail(c, CRUX_EINVAL, "%s: n_policy = %lld must leave policy and demo rows in a batch of %lld", who, (long long)Bp, (long long)B);
  if (gp && Be != Bp) return crux_fail(c, CRUX_EINVAL, "%s: the gradient penalty needs as many demo rows as policy rows (%lld, %lld)", who, (long long)Be, (long long)Bp);
  if (reg && !(alpha_reg > 0.f)) return crux_fail(c, CRUX_EINVAL, "%s: alpha_reg must be > 0", who);
  const int64_t H = gp ? Be : 0, NC = 2 * B + H;
  if (NC > (1 << 20))      // the forward pass covers s, s' and the penalty columns at once; the dense engine takes at most 2^20 columns
    return crux_fail(c, CRUX_EINVAL, "%s: batch %lld gives %lld columns (s, s'%s), more than the 2^20 one forward pass takes", who, (long long)B, (long long)NC, gp ? " and the penalty's" : "");
  IqBufs ib{}; rc = iq_prepare(q, B, H, gp != 0, ib, who); if (rc) return rc;
  const float* S = (const float*)b->col[CRUX_COL_S];
  hipLaunchKernelGGL(k_iq_expand, dim3(nblk(NC)), dim3(256), 0, c->stream, S, (const float*)b->col[CRUX_COL_SP], B, S + Bp * od, S, H, od, seed, counter, ib.X, ib.nanflag);
  rc = crux_launch_check(c, "k_iq_expand"); if (rc) return rc;
  rc = crux_dense_forward(q, ib.X, NC, c->stream); if (rc) return rc;
  if (H) { const int64_t ny = (int64_t)A * H; crux_launch<FillOp>(nblk(ny), 256, c->stream, ib.dy + 2 * B * A, 1.0f, ny); }
  hipLaunchKernelGGL(k_iq_head, dim3(1), dim3(256), 0, c->stream, (const float*)crux_dense_act(q, nd.L), (const uint8_t*)b->col[CRUX_COL_A], (const uint8_t*)b->col[CRUX_COL_DONE],
                     A, B, Bp, gamma_iq, reg, alpha_reg, (const int32_t*)ib.nanflag, ib.dy, ib.stats);
  rc = crux_launch_check(c, "k_iq_head"); if (rc) return rc;
  rc = iq_dgrad(q, B, H, ib); if (rc) return rc;
  for (int l = 1; l <= nd.L; ++l) {       // the loss's weight gradient over the s and s' columns only
    const float* hx = l == 1 ? ib.X : crux_dense_act(q, l - 1);
    rc = iq_wgrad(c, ib.Z[l], hx, nd.dims[l], nd.dims[l - 1], 2 * B, q->g + nd.woff[l - 1], q->g + nd.boff[l - 1]); if (rc) return rc;
  }
  if (H) {
    hipLaunchKernelGGL(k_iq_gp_head, dim3(1), dim3(256), 0, c->stream, (const float*)(ib.G[0] + 2 * B * od), od, H, 1.0f, lambda_gp, (const int32_t*)ib.nanflag, ib.gb[0], ib.stats);
    rc = crux_launch_check(c, "k_iq_gp_head"); if (rc) return rc;
    rc = iq_penalty_sweeps(q, B, H, ib); if (rc) return rc;
    rc = iq_add_penalty(q, ib); if (rc) return rc;
  }
  crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, q->g, (int64_t)nd.n_params, (float*)nullptr, (int64_t)0, ib.ssq, Sumsq2Fix{});
  hipLaunchKernelGGL(k_iq_info, dim3(1), dim3(1), 0, c->stream, (const double*)ib.stats, (const double*)ib.ssq, B, Bp, H, gp, lambda_gp, reg, alpha_reg, ib.dinfo, ib.extra);
  rc = crux_launch_check(c, "k_iq_info"); if (rc) return rc;
  rc = adam_gated(q, ib.ssq, ib.status); if (rc) return rc;
  return finish_step(c, ib.dinfo, ib.extra, 6, ib.status, info_out, iq_out, who);
}

}  // extern "C"
