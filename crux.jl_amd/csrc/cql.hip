// cql.hip -- offline RL: the conservative critic term of CQL (src/model_free/batch/cql.jl) on the dense engine (dense.hip) and SAC's pieces (sac.hip).
// Reference: conservative_loss cql.jl:24-35, cql_critic_loss = double_Q_loss + conservative_loss, cql_alpha_loss = -conservative_loss on fresh samples;
// train! src/training.jl:13-25 (gradient norm, NaN => error before the update, Adam).
//
// One call of the conservative term for a minibatch of B states and N action samples per source:
//   k_cql_expand   SA = [vcat(s, a_data) | vcat(s, a_pi(k)) k = 1..N | vcat(s, a_unif(k)) k = 1..N], one (od+ad) x (1+2N)B matrix, + the 2N B logprobs
//   dense forward  Q1 and Q2 over all (1+2N)B columns: one launch per layer and net (no per-sample loop)
//   k_cql_head     per state c_k = mean(Q1, Q2)(s, a_k) - logprob_k, lse = m + log sum exp(c_k - m) over k ascending, softmax weights -> dL/dQ seeds and the reductions
//   backward       weight gradients through the wide-K GEMM below (K = (1+2N)B columns), data gradients through the existing tile GEMM
// Randomness: include/crux_rng.h (CQL paragraph). The samples are drawn without gradient (ignore_derivatives, cql.jl:26-29): nothing reaches the actor.
#include "common.h"
#include "exec.h"

// ---- the SA matrix of all (1 + 2N) B columns ---------------------------------------------------------------------------------------------------------------------
// column col = blk * B + j: blk 0 the data action, blk 1..N policy sample k = blk - 1 (exploration(pi, s), GaussExploreOp's arithmetic), blk N+1..2N uniform sample
// k = blk - 1 - N (Float32.(rand(Product(Uniform(lo, hi))))). stream = (k B + j) ad + d for both kinds (the SAC streams j ad + d are the k = 0 case).
__global__ __launch_bounds__(256) void k_cql_expand(const float* __restrict__ mu, const float* __restrict__ ls, const float* __restrict__ s, const float* __restrict__ a,
                                                    int od, int ad, int64_t B, int N, float lo, float hi, uint64_t seed, uint64_t counter,
                                                    float* __restrict__ sa, float* __restrict__ lp, float* __restrict__ samples, int32_t* __restrict__ nanflag) {
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (col >= (int64_t)(1 + 2 * N) * B) return;
  const int blk = (int)(col / B); const int64_t j = col - (int64_t)blk * B; const int sd = od + ad;
  float* o = sa + col * sd;
  for (int k = 0; k < od; ++k) o[k] = s[j * od + k];
  const int64_t q = col - B;                                            // (blk - 1) B + j: the sample's slot in lp / samples
  if (blk == 0) {
    for (int d = 0; d < ad; ++d) o[od + d] = a[j * ad + d];
  } else if (blk <= N) {
    const int k = blk - 1; float acc = 0.f;
    for (int d = 0; d < ad; ++d) {                                      // GaussExploreOp (sac.hip), stream (k B + j) ad + d
      const float sg = expf(ls[d]); const float e = sac_randn(seed, counter, (uint32_t)(((int64_t)k * B + j) * ad + d));
      const float m = mu[j * ad + d]; const float av = __fadd_rn(__fmul_rn(e, sg), m);
      const float s2 = __fmul_rn(sg, sg), df = __fsub_rn(av, m);
      acc = __fadd_rn(acc, __fsub_rn(__fsub_rn(-(__fmul_rn(df, df)) / __fmul_rn(2.f, s2), 0.9189385332046727f), ls[d]));
      o[od + d] = av; if (samples) samples[q * ad + d] = av;
    }
    lp[q] = acc;
  } else {
    const int k = blk - 1 - N; const double dlo = (double)lo, w = (double)hi - (double)lo;
    for (int d = 0; d < ad; ++d) {
      const crux_u32x4 x = crux_philox(seed, counter, (uint32_t)(((int64_t)k * B + j) * ad + d), CRUX_RNG_CQL_UNIFORM);
      const float av = (float)(dlo + w * crux_u32x2_to_f64(x.v[0], x.v[1]));
      o[od + d] = av; if (samples) samples[q * ad + d] = av;
    }
    lp[q] = (float)(-(double)ad * log(w));                             // logpdf of the product: ad terms of -log(hi - lo), summed in Float64
  }
  // A NaN in the column (a state, a data action, a sample or its logprob) makes Q and the loss NaN in the reference (NNlib's relu(NaN) = max(0, NaN) is NaN); the
  // dense engine's relu maps NaN to 0, so the head is told instead and poisons what it forms (nanflag[0], read by k_cql_head)
  bool bad = blk > 0 && lp[q] != lp[q];
  for (int r = 0; r < sd; ++r) bad = bad || o[r] != o[r];
  if (bad) atomicOr((int*)nanflag, 1);
}

// The same matrix for a two-headed actor (crux_mlp_set_sigma_head): z = actor(s) [2 ad x B], mu = z[d], logSigma(s) = z[ad + d]. Policy sample k of column j restates
// SigmaExploreOp (sac.hip) operation for operation on the stream (k B + j) ad + d, so block k = 0 and its logprob are crux_sigma_head_explore's bits; ascale > 0 is the
// squashed head (sigma = exp(clamp(l, -5, 2)), a = ascale tanh(u), the tanh correction, -l unclamped: policies.jl:374-396). Data and uniform blocks as in k_cql_expand.
__global__ __launch_bounds__(256) void k_cql_expand_sigma(const float* __restrict__ z, const float* __restrict__ s, const float* __restrict__ a, int od, int ad, int64_t B, int N, float ascale,
                                                          float lo, float hi, uint64_t seed, uint64_t counter, float* __restrict__ sa, float* __restrict__ lp, float* __restrict__ samples,
                                                          int32_t* __restrict__ nanflag) {
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (col >= (int64_t)(1 + 2 * N) * B) return;
  const int blk = (int)(col / B); const int64_t j = col - (int64_t)blk * B; const int sd = od + ad;
  float* o = sa + col * sd;
  for (int k = 0; k < od; ++k) o[k] = s[j * od + k];
  const int64_t q = col - B;                                            // (blk - 1) B + j: the sample's slot in lp / samples
  if (blk == 0) {
    for (int d = 0; d < ad; ++d) o[od + d] = a[j * ad + d];
  } else if (blk <= N) {
    const int k = blk - 1; const float* zj = z + j * 2 * ad; float acc = 0.f;
    for (int d = 0; d < ad; ++d) {                                      // SigmaExploreOp (sac.hip), stream (k B + j) ad + d
      const float m = zj[d], l = zj[ad + d]; const float sg = expf(ascale > 0.f ? sq_clampls(l) : l);
      const float e = sac_randn(seed, counter, (uint32_t)(((int64_t)k * B + j) * ad + d));
      const float u = __fadd_rn(__fmul_rn(e, sg), m); const float s2 = __fmul_rn(sg, sg), df = __fsub_rn(u, m);
      float t = __fsub_rn(__fsub_rn(-(__fmul_rn(df, df)) / __fmul_rn(2.f, s2), 0.9189385332046727f), l);
      if (ascale > 0.f) t = __fsub_rn(t, sq_corr(u));
      acc = __fadd_rn(acc, t);
      const float av = ascale > 0.f ? __fmul_rn(ascale, tanhf(u)) : u;
      o[od + d] = av; if (samples) samples[q * ad + d] = av;
    }
    lp[q] = acc;
  } else {
    const int k = blk - 1 - N; const double dlo = (double)lo, w = (double)hi - (double)lo;
    for (int d = 0; d < ad; ++d) {
      const crux_u32x4 x = crux_philox(seed, counter, (uint32_t)(((int64_t)k * B + j) * ad + d), CRUX_RNG_CQL_UNIFORM);
      const float av = (float)(dlo + w * crux_u32x2_to_f64(x.v[0], x.v[1]));
      o[od + d] = av; if (samples) samples[q * ad + d] = av;
    }
    lp[q] = (float)(-(double)ad * log(w));
  }
  bool bad = blk > 0 && lp[q] != lp[q];                                  // the NaN flag of k_cql_expand
  for (int r = 0; r < sd; ++r) bad = bad || o[r] != o[r];
  if (bad) atomicOr((int*)nanflag, 1);
}

// ---- the head: log-sum-exp over the 2N samples of every state, dL/dQ seeds, reductions (one block of 256, fixed order) -------------------------------------------
// stats: [0] mean lse, [1] mean qbar(s, a_data), [2] beta, [3] beta (5 L - thresh), [4] double_Q_loss, [5] Q1avg, [6] Q2avg, [7] exp(log_alpha) (unclamped)
// dy (critic step only): sample columns 5 beta 0.5 softmax_k / B for both nets; data columns 0.5 * 2 (Q_t - y) w / B - 5 beta 0.5 / B
__global__ __launch_bounds__(256) void k_cql_head(const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ lp, const float* __restrict__ y, const float* __restrict__ w,
                                                  int64_t B, int N, const float* __restrict__ log_alpha, float thresh, float* __restrict__ dy1, float* __restrict__ dy2, double* __restrict__ stats,
                                                  const int32_t* __restrict__ nanflag) {
  __shared__ double red[4];
  const float ea = expf(log_alpha[0]); const float beta = fminf(fmaxf(ea, 0.f), 1e6f); const bool poison = nanflag[0] != 0;
  const float invB = 1.f / (float)B; const float gs = 5.f * beta * 0.5f * invB;
  double s_lse = 0, s_qd = 0, s_l1 = 0, s_l2 = 0, s_q1 = 0, s_q2 = 0;
  for (int64_t j = threadIdx.x; j < B; j += 256) {
    float m = -INFINITY;
    for (int k = 0; k < 2 * N; ++k) { const int64_t col = (int64_t)(1 + k) * B + j; const float ck = (q1[col] + q2[col]) * 0.5f - lp[(int64_t)k * B + j]; m = fmaxf(m, ck); }
    float se = 0.f;
    for (int k = 0; k < 2 * N; ++k) { const int64_t col = (int64_t)(1 + k) * B + j; const float ck = (q1[col] + q2[col]) * 0.5f - lp[(int64_t)k * B + j]; se += expf(ck - m); }
    const float lse = poison ? NAN : m + logf(se);
    if (dy1) for (int k = 0; k < 2 * N; ++k) { const int64_t col = (int64_t)(1 + k) * B + j; const float ck = (q1[col] + q2[col]) * 0.5f - lp[(int64_t)k * B + j];
      const float g = poison ? NAN : gs * (expf(ck - m) / se); dy1[col] = g; dy2[col] = g; }
    const float qd = poison ? NAN : (q1[j] + q2[j]) * 0.5f;
    s_lse += (double)lse; s_qd += (double)qd; s_q1 += (double)q1[j]; s_q2 += (double)q2[j];
    if (y) { const float ww = w ? w[j] : 1.f; const float d1 = q1[j] - y[j], d2 = q2[j] - y[j];
      s_l1 += (double)(d1 * d1 * ww); s_l2 += (double)(d2 * d2 * ww);
      if (dy1) { dy1[j] = 0.5f * (2.f * d1 * ww * invB) - gs; dy2[j] = 0.5f * (2.f * d2 * ww * invB) - gs; } }
  }
  s_lse = block_sum256(s_lse, red); s_qd = block_sum256(s_qd, red); s_l1 = block_sum256(s_l1, red); s_l2 = block_sum256(s_l2, red);
  s_q1 = block_sum256(s_q1, red); s_q2 = block_sum256(s_q2, red);
  if (threadIdx.x == 0) {
    const double ml = s_lse / (double)B, mq = s_qd / (double)B; const float Lc = (float)ml - (float)mq;
    stats[0] = ml; stats[1] = mq; stats[2] = beta; stats[3] = (double)(beta * (5.f * Lc - thresh));
    stats[4] = 0.5 * (s_l1 / (double)B) + 0.5 * (s_l2 / (double)B); stats[5] = s_q1 / (double)B; stats[6] = s_q2 / (double)B; stats[7] = ea;
  }
}
// the critic step's info row: LOSS = double_Q_loss + conservative_loss, GRAD_NORM, Q1AVG, Q2AVG
__global__ void k_cql_critic_info(const double* __restrict__ st, const double* __restrict__ ssq, float* __restrict__ dinfo) {
  if (threadIdx.x != 0) return;
  ssq_finalize(ssq);
  dinfo[CRUX_INFO_LOSS] = (float)st[4] + (float)st[3]; dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(ssq[0]);
  dinfo[CRUX_INFO_Q1AVG] = (float)st[5]; dinfo[CRUX_INFO_Q2AVG] = (float)st[6];
}
// cql_alpha_loss = -beta (5 L - thresh), beta = clamp(exp(x), 0, 1f6): d/dx = -exp(x) (5 L - thresh) inside the clamp, 0 beyond it. ssq[0] = g^2 (the NaN gate of Adam).
__global__ void k_cql_alpha_head(const double* __restrict__ st, const float* __restrict__ log_alpha, float thresh, float* __restrict__ g, double* __restrict__ ssq, float* __restrict__ dinfo) {
  if (threadIdx.x != 0) return;
  const float ea = expf(log_alpha[0]); const float Lc = (float)st[0] - (float)st[1];
  const float gv = ea <= 1e6f ? -(ea * (5.f * Lc - thresh)) : 0.f * Lc;        // (0 * NaN: a NaN loss still stops the update)
  g[0] = gv; ssq[0] = (double)gv * (double)gv;
  dinfo[CRUX_INFO_LOSS] = -(float)st[3]; dinfo[CRUX_INFO_GRAD_NORM] = fabsf(gv); dinfo[CRUX_INFO_ALPHA] = ea;
}

// ---- wide-K weight gradient: dW[i, j] = scale sum_s dZ[i, s] X[j, s], db[i] = scale sum_s dZ[i, s] over K = (1+2N)B columns ------------------------------------
// Gemm16's EPI_WGRAD splits K at most four ways inside one workgroup: at K = 5 376 every wave would walk the whole depth. Here K is cut into chunks of CQL_KC columns
// that run in different workgroups (one wave per 32 x 32 output block and chunk, 2 x 2 MFMA 16x16x4 f32 tiles sharing their operand loads); each chunk's partial goes
// to scratch and k_cql_wgrad_reduce adds the chunks in ascending order (deterministic: no atomics). db rides along in the waves of the first column block.
#define CQL_KC 256
__global__ __launch_bounds__(256) void k_cql_wgrad_part(const float* __restrict__ dZ, const float* __restrict__ X, int M, int N, int K, int want_db, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int bm = (M + 31) >> 5, bn = (N + 31) >> 5, nbt = bm * bn, P = (K + CQL_KC - 1) / CQL_KC;
  const int wid = (int)blockIdx.x * 4 + wv; if (wid >= nbt * P) return;
  const int bt = wid % nbt, p = wid / nbt;
  const int i0 = (bt % bm) << 5, j0 = (bt / bm) << 5;
  const int kbeg = p * CQL_KC, kend = kbeg + CQL_KC < K ? kbeg + CQL_KC : K;
  const int ia0 = i0 + c, ia1 = i0 + 16 + c, jb0 = j0 + c, jb1 = j0 + 16 + c;
  const bool va0 = ia0 < M, va1 = ia1 < M, vb0 = jb0 < N, vb1 = jb1 < N;
  f32x4 acc00 = {0.f, 0.f, 0.f, 0.f}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
  float prow0 = 0.f, prow1 = 0.f; const bool rows = want_db && j0 == 0;
  for (int k0 = kbeg; k0 < kend; k0 += 16) {
    float a0[4], a1[4], b0[4], b1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {       // lane group g supplies k = k0 + 4g + r to MFMA r (both operands agree)
      const int kk = k0 + 4 * g + r; const bool ok = kk < kend; const int64_t za = (int64_t)kk * M, xb = (int64_t)kk * N;
      a0[r] = (ok && va0) ? dZ[ia0 + za] : 0.f; a1[r] = (ok && va1) ? dZ[ia1 + za] : 0.f;
      b0[r] = (ok && vb0) ? X[jb0 + xb] : 0.f;  b1[r] = (ok && vb1) ? X[jb1 + xb] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[r], b0[r], acc00, 0, 0, 0); acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[r], b1[r], acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[r], b0[r], acc10, 0, 0, 0); acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[r], b1[r], acc11, 0, 0, 0);
    }
    if (rows) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { prow0 += a0[r]; prow1 += a1[r]; }
    }
  }
  const int64_t stride = (int64_t)M * N + M; float* pp = part + (int64_t)p * stride;
  // D layout: reg r <-> row 4g + r, column c of the 16 x 16 tile
  auto store = [&](const f32x4& acc, int ib, int jj) {
    if (jj >= N) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int i = ib + 4 * g + r; if (i < M) pp[i + (int64_t)jj * M] = acc[r]; } };
  store(acc00, i0, jb0); store(acc01, i0, jb1); store(acc10, i0 + 16, jb0); store(acc11, i0 + 16, jb1);
  if (rows) {          // lanes c, c+16, c+32, c+48 hold the four k groups of row i0 + c (+16): fixed-order combine
    prow0 += __shfl_xor(prow0, 16, 64); prow0 += __shfl_xor(prow0, 32, 64);
    prow1 += __shfl_xor(prow1, 16, 64); prow1 += __shfl_xor(prow1, 32, 64);
    if (g == 0) { if (va0) pp[(int64_t)M * N + ia0] = prow0; if (va1) pp[(int64_t)M * N + ia1] = prow1; }
  }
}
__global__ __launch_bounds__(256) void k_cql_wgrad_reduce(const float* __restrict__ part, int64_t MN, int64_t M, int P, float scale, float* __restrict__ dW, float* __restrict__ db) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; const int64_t stride = MN + M; if (e >= stride) return;
  float v = 0.f;
  for (int p = 0; p < P; ++p) v += part[(int64_t)p * stride + e];
  v *= scale;
  if (e < MN) dW[e] = v; else db[e - MN] = v;
}
static inline size_t cql_wgrad_floats(int M, int N, int64_t K) { return (size_t)((K + CQL_KC - 1) / CQL_KC) * ((size_t)M * N + M); }
static int32_t cql_wgrad(crux_ctx* c, const float* dZ, const float* X, int M, int N, int64_t K, float* part, float* dW, float* db, hipStream_t st) {
  const int P = (int)((K + CQL_KC - 1) / CQL_KC); const int64_t waves = (int64_t)((M + 31) >> 5) * ((N + 31) >> 5) * P;
  hipLaunchKernelGGL(k_cql_wgrad_part, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, dZ, X, M, N, (int)K, 1, part);
  const int64_t n = (int64_t)M * N + M;
  hipLaunchKernelGGL(k_cql_wgrad_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)part, (int64_t)M * N, (int64_t)M, P, 1.0f, dW, db);
  return crux_launch_check(c, "k_cql_wgrad");
}

// reverse pass of one net over the NB columns of SA after crux_dense_forward(n, sa, NB): parameter gradients only (the input gradient is not needed: the samples carry none)
static int32_t cql_backward(crux_mlp* n, const float* sa, int64_t NB, const float* d_dy, float* part, hipStream_t st) {
  crux_ctx* c = n->ctx; const NetDesc& nd = n->nd;
  const float* dcur = d_dy; float* dnxt = ws_delta(n, 0); float* dspare = ws_delta(n, 1);
  if (nd.acts[nd.L - 1] != CRUX_ACT_IDENTITY) {
    const int64_t cnt = (int64_t)nd.dims[nd.L] * NB;
    crux_launch<ActGradOp>((unsigned)((cnt + 255) / 256), 256, st, d_dy, (const float*)crux_dense_act(n, nd.L), nd.acts[nd.L - 1], cnt, dnxt);
    dcur = dnxt; dnxt = dspare; dspare = const_cast<float*>(dcur);
  }
  for (int l = nd.L - 1; l >= 0; --l) {
    const int in = nd.dims[l], out = nd.dims[l + 1];
    const float* x = l == 0 ? sa : crux_dense_act(n, l);
    int32_t rc = cql_wgrad(c, dcur, x, out, in, NB, part, n->g + nd.woff[l], n->g + nd.boff[l], st); if (rc) return rc;
    if (l > 0) {       // dX of the layer below through the existing tile GEMM (K = out is small; the width is in N)
      GemmArgs q{}; q.A = n->p + nd.woff[l]; q.sAi = out; q.sAk = 1; q.B = dcur; q.sBk = 1; q.sBj = out; q.M = in; q.N = (int)NB; q.K = out;
      q.C = dnxt; q.sCj = in; q.epi = EPI_BWD_DATA; q.ysrc = x; q.act = nd.acts[l - 1];
      rc = launch_gemm(c, q, st); if (rc) return rc;
      dcur = dnxt; float* t = dnxt; dnxt = dspare; dspare = t;
    }
  }
  return crux_launch_check(c, "cql backward");
}

// expand + forward of both nets + head: shared by the three entry points. dy1 / dy2 / y NULL: no seeds (alpha step, conservative value)
struct CqlBufs : StepSmall { float* sa; float* lp; float* dy1; float* dy2; float* part; };
static int32_t cql_ranges(crux_ctx* c, crux_buffer* b, int n_samples, float lo, float hi, const char* who) {
  if (n_samples < 1 || n_samples > 1024) return crux_fail(c, CRUX_EINVAL, "%s: CQL_n_action_samples = %d out of range [1, 1024]", who, n_samples);
  if (!(hi > lo)) return crux_fail(c, CRUX_EINVAL, "%s: the IS box needs lo < hi (got %g, %g)", who, (double)lo, (double)hi);
  const int64_t NB = (int64_t)(1 + 2 * n_samples) * b->elements;
  if (NB > (1 << 20) || (int64_t)2 * n_samples * b->elements * b->act_dim >= ((int64_t)1 << 32)) return crux_fail(c, CRUX_EINVAL, "%s: (1 + 2N) B = %lld columns is too many", who, (long long)NB);
  return CRUX_OK;
}
static int32_t cql_check(crux_ctx* c, crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int n_samples, float lo, float hi, const char* who) {
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  // check_sac takes a two-headed actor (crux_mlp_set_sigma_head) for the SAC entries; k_cql_expand reads a constant logSigma from the extras and [ad x B] means, so not here
  if (actor && actor->sigma_head) return crux_fail(c, CRUX_EUNSUP, "%s: CQL's sampled-action terms are not implemented for a two-headed actor (logSigma network); use a constant logSigma", who);
  int32_t rc = check_sac(c, actor, q1, q2, la, b, who); if (rc) return rc;
  return cql_ranges(c, b, n_samples, lo, hi, who);
}
// the _sigma entries: a two-headed actor only ("not two-headed" is sigma_head_check's CRUX_EINVAL), then check_sac's two-headed branch (od -> 2 ad, no extras, ad <= 64)
static int32_t cql_check_sigma(crux_ctx* c, crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int n_samples, float lo, float hi, const char* who) {
  if (!actor->sigma_head) return crux_fail(c, CRUX_EINVAL, "%s: the actor handle is not two-headed (crux_mlp_set_sigma_head); the plain entry takes a constant logSigma", who);
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  int32_t rc = check_sac(c, actor, q1, q2, la, b, who); if (rc) return rc;
  return cql_ranges(c, b, n_samples, lo, hi, who);
}
static int32_t cql_prepare(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_buffer* b, int N, bool seeds, CqlBufs& cb, const char* who) {
  crux_ctx* c = actor->ctx; const int64_t B = b->elements; const int od = b->obs_dim, ad = b->act_dim, sd = od + ad; const int64_t NB = (int64_t)(1 + 2 * N) * B;
  size_t pf = 0;
  if (seeds) { const crux_mlp* qs[2] = {q1, q2};
    for (int t = 0; t < 2; ++t) for (int l = 0; l < qs[t]->nd.L; ++l) { const size_t f = cql_wgrad_floats(qs[t]->nd.dims[l + 1], qs[t]->nd.dims[l], NB); if (f > pf) pf = f; } }
  const size_t bytes = 4 * ((size_t)NB * sd + (size_t)2 * N * B + (seeds ? 2 * (size_t)NB : 0) + pf) + 6 * 256 + STEP_SMALL;     // + the rounding of six takes
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  cb.sa = cv.take<float>((size_t)NB * sd); cb.lp = cv.take<float>((size_t)2 * N * B);
  cb.dy1 = seeds ? cv.take<float>((size_t)NB) : nullptr; cb.dy2 = seeds ? cv.take<float>((size_t)NB) : nullptr; cb.part = seeds ? cv.take<float>(pf) : nullptr;
  return step_small(c, cv, cb);
}
static int32_t cql_forward_head(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int N, float lo, float hi, float thresh, const float* d_y, int32_t use_weight,
                                uint64_t seed, uint64_t counter, const CqlBufs& cb, float* d_samples, float* d_lp_out) {
  crux_ctx* c = actor->ctx; const int64_t B = b->elements; const int od = b->obs_dim, ad = b->act_dim; const int64_t NB = (int64_t)(1 + 2 * N) * B;
  const float* S = (const float*)b->col[CRUX_COL_S];
  int32_t rc = crux_dense_forward(actor, S, B, c->stream); if (rc) return rc;          // the means; mu does not depend on k
  if (actor->sigma_head)       // [mu; logSigma(s)] from the one forward pass (the _sigma entries only: cql_check refuses the flag)
    hipLaunchKernelGGL(k_cql_expand_sigma, dim3(nblk(NB)), dim3(256), 0, c->stream, (const float*)crux_dense_act(actor, actor->nd.L), S, (const float*)b->col[CRUX_COL_A], od, ad, B, N,
                       actor->squash, lo, hi, seed, counter, cb.sa, cb.lp, d_samples, cb.nanflag);
  else
    hipLaunchKernelGGL(k_cql_expand, dim3(nblk(NB)), dim3(256), 0, c->stream, (const float*)crux_dense_act(actor, actor->nd.L), (const float*)(actor->p + actor->nd.xoff), S,
                       (const float*)b->col[CRUX_COL_A], od, ad, B, N, lo, hi, seed, counter, cb.sa, cb.lp, d_samples, cb.nanflag);
  rc = crux_launch_check(c, "k_cql_expand"); if (rc) return rc;
  rc = crux_dense_forward(q1, cb.sa, NB, c->stream); if (rc) return rc;
  rc = crux_dense_forward(q2, cb.sa, NB, c->stream); if (rc) return rc;
  const float* w = (d_y && use_weight) ? (const float*)b->col[CRUX_COL_WEIGHT] : nullptr;
  hipLaunchKernelGGL(k_cql_head, dim3(1), dim3(256), 0, c->stream, (const float*)crux_dense_act(q1, q1->nd.L), (const float*)crux_dense_act(q2, q2->nd.L), (const float*)cb.lp, d_y, w,
                     B, N, (const float*)la->p, thresh, cb.dy1, cb.dy2, cb.stats, (const int32_t*)cb.nanflag);
  if (d_lp_out) HIPCHK(c, hipMemcpyAsync(d_lp_out, cb.lp, sizeof(float) * (size_t)2 * N * B, hipMemcpyDeviceToDevice, c->stream));
  return crux_launch_check(c, "k_cql_head");
}

// the bodies of the entry points: check = cql_check (constant logSigma extras) or cql_check_sigma (two-headed actor, the _sigma entries); everything behind the expansion is shared
typedef int32_t (*CqlCheck)(crux_ctx*, crux_mlp*, crux_mlp*, crux_mlp*, crux_mlp*, crux_buffer*, int, float, float, const char*);
static int32_t cql_critic_step(CqlCheck check, const char* entry, crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, const float* d_y, int32_t n_samples, float is_lo, float is_hi,
                             float thresh, int32_t use_weight, uint64_t seed, uint64_t counter, float* info_out) { CRUX_PLAIN_ONLY(entry, actor, q1, q2, la);
  if (!actor || !q1 || !q2 || !la || !b || !d_y) return CRUX_EINVAL;
  crux_ctx* c = actor->ctx; const char* who = "cql_critic_loss";
  int32_t rc = check(c, actor, q1, q2, la, b, n_samples, is_lo, is_hi, who); if (rc) return rc;
  if (use_weight && !has_col(b, CRUX_COL_WEIGHT)) return crux_fail(c, CRUX_EINVAL, "%s(weight=:weight): batch has no :weight column", who);
  CqlBufs cb{}; rc = cql_prepare(actor, q1, q2, b, n_samples, true, cb, who); if (rc) return rc;
  rc = cql_forward_head(actor, q1, q2, la, b, n_samples, is_lo, is_hi, thresh, d_y, use_weight, seed, counter, cb, nullptr, nullptr); if (rc) return rc;
  const int64_t NB = (int64_t)(1 + 2 * n_samples) * b->elements;
  rc = cql_backward(q1, cb.sa, NB, cb.dy1, cb.part, c->stream); if (rc) return rc;
  rc = cql_backward(q2, cb.sa, NB, cb.dy2, cb.part, c->stream); if (rc) return rc;
  crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, q1->g, (int64_t)q1->nd.n_params, q2->g, (int64_t)q2->nd.n_params, cb.ssq, Sumsq2Fix{});
  hipLaunchKernelGGL(k_cql_critic_info, dim3(1), dim3(1), 0, c->stream, (const double*)cb.stats, (const double*)cb.ssq, cb.dinfo);
  rc = adam_gated(q1, cb.ssq, cb.status); if (rc) return rc;
  rc = adam_gated(q2, cb.ssq, cb.status); if (rc) return rc;
  return finish_step(c, cb.dinfo, cb.status, info_out, who);
}

static int32_t cql_alpha_step(CqlCheck check, const char* entry, crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int32_t n_samples, float is_lo, float is_hi, float thresh,
                            uint64_t seed, uint64_t counter, float* info_out) { CRUX_PLAIN_ONLY(entry, actor, q1, q2, la);
  if (!actor || !q1 || !q2 || !la || !b) return CRUX_EINVAL;
  crux_ctx* c = actor->ctx; const char* who = "cql_alpha_loss";
  int32_t rc = check(c, actor, q1, q2, la, b, n_samples, is_lo, is_hi, who); if (rc) return rc;
  CqlBufs cb{}; rc = cql_prepare(actor, q1, q2, b, n_samples, false, cb, who); if (rc) return rc;
  rc = cql_forward_head(actor, q1, q2, la, b, n_samples, is_lo, is_hi, thresh, nullptr, 0, seed, counter, cb, nullptr, nullptr); if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(la->g, 0, sizeof(float) * (size_t)la->nd.n_params, c->stream));
  hipLaunchKernelGGL(k_cql_alpha_head, dim3(1), dim3(1), 0, c->stream, (const double*)cb.stats, (const float*)la->p, thresh, la->g, cb.ssq, cb.dinfo);
  rc = crux_launch_check(c, "k_cql_alpha_head"); if (rc) return rc;
  rc = adam_gated(la, cb.ssq, cb.status, false); if (rc) return rc;
  return finish_step(c, cb.dinfo, cb.status, info_out, who);
}

static int32_t cql_conservative(CqlCheck check, const char* entry, crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int32_t n_samples, float is_lo, float is_hi, float thresh,
                              uint64_t seed, uint64_t counter, float* out4, float* d_samples, float* d_logprobs) { CRUX_PLAIN_ONLY(entry, actor, q1, q2, la);
  if (!actor || !q1 || !q2 || !la || !b || !out4) return CRUX_EINVAL;
  crux_ctx* c = actor->ctx; const char* who = "conservative_loss";
  int32_t rc = check(c, actor, q1, q2, la, b, n_samples, is_lo, is_hi, who); if (rc) return rc;
  CqlBufs cb{}; rc = cql_prepare(actor, q1, q2, b, n_samples, false, cb, who); if (rc) return rc;
  rc = cql_forward_head(actor, q1, q2, la, b, n_samples, is_lo, is_hi, thresh, nullptr, 0, seed, counter, cb, d_samples, d_logprobs); if (rc) return rc;
  double h[8];
  HIPCHK(c, hipMemcpyAsync(h, cb.stats, sizeof h, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  out4[0] = (float)h[0]; out4[1] = (float)h[1]; out4[2] = (float)h[2]; out4[3] = (float)h[3];
  return CRUX_OK;
}

extern "C" {

int32_t crux_cql_critic_step(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, const float* d_y, int32_t n_samples, float is_lo, float is_hi,
                             float thresh, int32_t use_weight, uint64_t seed, uint64_t counter, float* info_out) {
  return cql_critic_step(cql_check, "crux_cql_critic_step", actor, q1, q2, la, b, d_y, n_samples, is_lo, is_hi, thresh, use_weight, seed, counter, info_out);
}
int32_t crux_cql_alpha_step(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int32_t n_samples, float is_lo, float is_hi, float thresh,
                            uint64_t seed, uint64_t counter, float* info_out) {
  return cql_alpha_step(cql_check, "crux_cql_alpha_step", actor, q1, q2, la, b, n_samples, is_lo, is_hi, thresh, seed, counter, info_out);
}
int32_t crux_cql_conservative(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int32_t n_samples, float is_lo, float is_hi, float thresh,
                              uint64_t seed, uint64_t counter, float* out4, float* d_samples, float* d_logprobs) {
  return cql_conservative(cql_check, "crux_cql_conservative", actor, q1, q2, la, b, n_samples, is_lo, is_hi, thresh, seed, counter, out4, d_samples, d_logprobs);
}
// the same three for a two-headed actor (crux_mlp_set_sigma_head): k_cql_expand_sigma draws the policy samples; CRUX_EINVAL for a handle without the flag
int32_t crux_cql_critic_step_sigma(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, const float* d_y, int32_t n_samples, float is_lo, float is_hi,
                                   float thresh, int32_t use_weight, uint64_t seed, uint64_t counter, float* info_out) {
  return cql_critic_step(cql_check_sigma, "crux_cql_critic_step_sigma", actor, q1, q2, la, b, d_y, n_samples, is_lo, is_hi, thresh, use_weight, seed, counter, info_out);
}
int32_t crux_cql_alpha_step_sigma(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int32_t n_samples, float is_lo, float is_hi, float thresh,
                                  uint64_t seed, uint64_t counter, float* info_out) {
  return cql_alpha_step(cql_check_sigma, "crux_cql_alpha_step_sigma", actor, q1, q2, la, b, n_samples, is_lo, is_hi, thresh, seed, counter, info_out);
}
int32_t crux_cql_conservative_sigma(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, int32_t n_samples, float is_lo, float is_hi, float thresh,
                                    uint64_t seed, uint64_t counter, float* out4, float* d_samples, float* d_logprobs) {
  return cql_conservative(cql_check_sigma, "crux_cql_conservative_sigma", actor, q1, q2, la, b, n_samples, is_lo, is_hi, thresh, seed, counter, out4, d_samples, d_logprobs);
}

}  // extern "C"
