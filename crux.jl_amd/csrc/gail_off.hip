// gail_off.hip -- off-policy adversarial imitation on the dense engine (dense.hip): the discriminator step, the round and the reward rewrite of OffPolicyGAIL's
// GAIL_callback (src/model_free/il/off_policy_gail.jl:64-125) and AdRIL's ring relabel (src/model_free/il/AdRIL.jl:39-50). Reference of the update: train!
// src/training.jl:13-25 (gradient norm, NaN => error before the update, Adam).
//
// One discriminator step over K = 2 + N_nda sources and Bd columns each (NC = K Bd):
//   k_offgail_gather   row ids drawn on the device (crux_uniform_sample's draw: Philox(seed, counter Bd + j, 16 + k, SAMPLE), id = (x0 len) >> 32), X = [vcat(s, a)] with
//                      source k in columns [k Bd, (k + 1) Bd): demo, the solver's ring, NDA 1.. (:78, :81); only s and a are read; NaN anywhere -> nanflag
//   dense forward      D over all NC columns, activations cached
//   k_offgail_ce_head  logitcrossentropy(D(x), y), label of a column = its source (:87-98): L = mean_j (logsumexp z_j - z_j[label_j]), seed (softmax - onehot) / NC; fixed order
//   dense backward     the engine's data / weight gradient; then the norm, the info row, the NaN gate and Adam as every *_step
// The reward rewrite (:121-124): p = softmax(D(vcat(s, a))) over the staging batch, r = sum_k w_k (log(p_k + 1f-5) - log(1f0 - p_k + 1f-5)), w = [1, 0, -1/N_nda, ...].
// No float atomics anywhere: two identical calls give identical bits. The engine's relu maps NaN to 0 where NNlib's propagates it, so the gather flags NaN inputs and the head
// poisons what it forms (the idiom of k_iq_expand / k_iq_head).
// A round enqueues d_epochs steps and the reward rewrite back to back. All steps share one status word (chain.h: ChainHead, with each step's small region as its row), and
// k_offgail_reward writes nothing once it is set -- the round stops at that step without the host looking. The read-back and the report are chain.h's.
#include "common.h"
#include "exec.h"

#define OFFGAIL_MAXK 16
struct OgSrc { const float* s; const void* a; int64_t n; };

__global__ __launch_bounds__(256) void k_offgail_gather(const OgSrc* __restrict__ src, int u8, int od, int ad, int64_t Bd, uint64_t seed, uint64_t counter,
                                                        float* __restrict__ X, int32_t* __restrict__ nanflag) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (j >= Bd) return;
  const int k = blockIdx.y; const OgSrc q = src[k];
  const crux_u32x4 x = crux_philox(seed, counter * (uint64_t)Bd + (uint64_t)j, 16u + (uint32_t)k, CRUX_RNG_SAMPLE);
  const int64_t id = (int64_t)(((uint64_t)x.v[0] * (uint64_t)q.n) >> 32);      // < q.n <= the source's capacity
  float* o = X + ((int64_t)k * Bd + j) * (od + ad); bool bad = false;
  const float* s = q.s + id * od;
  for (int e = 0; e < od; ++e) { const float v = s[e]; o[e] = v; bad = bad || v != v; }
  if (u8) { const uint8_t* a = (const uint8_t*)q.a + id * ad; for (int e = 0; e < ad; ++e) o[od + e] = a[e] ? 1.f : 0.f; }
  else { const float* a = (const float*)q.a + id * ad; for (int e = 0; e < ad; ++e) { const float v = a[e]; o[od + e] = v; bad = bad || v != v; } }
  if (bad) atomicOr((int*)nanflag, 1);
}

// ---- labelled cross-entropy head (one block of 256, fixed order): z [K x NC], label of column j = j / Bd; stats[0] = sum_j (logsumexp z_j - z_j[label_j]) ------------
__global__ __launch_bounds__(256) void k_offgail_ce_head(const float* __restrict__ z, int K, int64_t Bd, int64_t NC, const int32_t* __restrict__ nanflag,
                                                         float* __restrict__ dz, double* __restrict__ stats) {
  __shared__ double red[4];
  const bool poison = nanflag[0] != 0; const float invN = 1.f / (float)NC;
  double sl = 0;
  for (int64_t j = threadIdx.x; j < NC; j += 256) {
    const float* q = z + j * K; float* d = dz + j * K; const int lab = (int)(j / Bd);
    float m = -INFINITY; for (int k = 0; k < K; ++k) m = fmaxf(m, q[k]);
    float se = 0.f; for (int k = 0; k < K; ++k) se += expf(q[k] - m);
    sl += (double)((m + logf(se)) - q[lab]);
    for (int k = 0; k < K; ++k) { const float g = (expf(q[k] - m) / se - (k == lab ? 1.f : 0.f)) * invN; d[k] = poison ? NAN : g; }
  }
  sl = block_sum256(sl, red);
  if (threadIdx.x == 0) stats[0] = poison ? NAN : sl;
}
__global__ void k_offgail_info(const double* __restrict__ st, const double* __restrict__ ssq, int64_t NC, float* __restrict__ dinfo) {
  if (threadIdx.x != 0) return;
  ssq_finalize(ssq);
  dinfo[CRUX_INFO_LOSS] = (float)(st[0] / (double)NC); dinfo[CRUX_INFO_GRAD_NORM] = (float)sqrt(ssq[0]);
}

// x = vcat(flatten(s), a) of the staging batch (value(D, s, a), :121); one-hot actions enter as 0/1
__global__ __launch_bounds__(256) void k_offgail_concat(const float* __restrict__ s, const void* __restrict__ a, int u8, int od, int ad, int64_t B, float* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; const int sd = od + ad; if (i >= B * sd) return;
  const int64_t j = i / sd; const int e = (int)(i - j * sd);
  x[i] = e < od ? s[j * od + e] : (u8 ? (((const uint8_t*)a)[j * ad + e - od] ? 1.f : 0.f) : ((const float*)a)[j * ad + e - od]);
}

// ---- the reward rewrite: z [K x B] discriminator outputs of the staging batch; partial[block] = sum of the rewards this block formed ---------------------------------
// Operand order as the reference writes it; the two logs, their difference, the weight and the sum over k are separate roundings (__fadd_rn / __fsub_rn / __fmul_rn: no
// contraction whatever the translation unit's -ffp-contract is). status (may be NULL): nothing is written once an earlier step of the round stopped with CRUX_ENAN.
#define OFFGAIL_RBLOCKS 64
__global__ __launch_bounds__(256) void k_offgail_reward(const float* __restrict__ z, int K, int64_t B, float w_nda, const int32_t* __restrict__ status,
                                                        float* __restrict__ r, double* __restrict__ partial) {
  __shared__ double red[4];
  const bool stop = status && status[0] == CRUX_ENAN;
  double s = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < B && !stop; j += (int64_t)gridDim.x * 256) {
    const float* q = z + j * K;
    float m = -INFINITY; for (int k = 0; k < K; ++k) m = fmaxf(m, q[k]);
    float se = 0.f; for (int k = 0; k < K; ++k) se += expf(q[k] - m);
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
      const float p = expf(q[k] - m) / se, w = k == 0 ? 1.f : (k == 1 ? 0.f : w_nda);
      const float t = __fmul_rn(__fsub_rn(logf(__fadd_rn(p, 1e-5f)), logf(__fadd_rn(__fsub_rn(1.f, p), 1e-5f))), w);
      acc = k == 0 ? t : __fadd_rn(acc, t);
    }
    r[j] = acc; s += (double)acc;
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---- AdRIL's relabel -------------------------------------------------------------------------------------------------------------------------------------------------
// maximum(ring[:i]) over len rows: per-block maxima (a maximum does not depend on the order it is formed in), combined in block order by every block of k_adril_relabel
#define ADRIL_BLOCKS 64
__global__ __launch_bounds__(256) void k_adril_max(const int64_t* __restrict__ ii, int64_t len, int64_t* __restrict__ part) {
  __shared__ int64_t red[4];
  int64_t m = INT64_MIN;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < len; p += (int64_t)gridDim.x * 256) m = ii[p] > m ? ii[p] : m;
  for (int o = 32; o > 0; o >>= 1) { const int64_t t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) { for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m; part[blockIdx.x] = m; }
}
// rows [first_new, first_new + n_new) mod cap are the block the rollout has just written: reward 0 (D[:r] .= 0, :40). Every other row: -1/k when i <= max_i - dN, else 0
// (:45-48). all_new: the reference's buffer was empty before its push (:42), nothing but the zeroing happens. out: {max_i, k, refused}
__global__ __launch_bounds__(256) void k_adril_relabel(const int64_t* __restrict__ ii, float* __restrict__ r, int64_t len, int64_t cap, int64_t first_new, int64_t n_new, int all_new,
                                                       int64_t buffer_init, int64_t dN, const int64_t* __restrict__ part, int64_t* __restrict__ out) {
  int64_t mx = part[0]; for (int b = 1; b < ADRIL_BLOCKS; ++b) mx = part[b] > mx ? part[b] : mx;
  const int64_t num = mx - buffer_init; const bool refused = !all_new && num % dN != 0;      // Int((max_i - buffer_init) / dN): InexactError
  const int64_t k = all_new ? 0 : num / dN - 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = mx; out[1] = k; out[2] = refused ? 1 : 0; }
  if (refused) return;
  const float rold = (float)(-1.0 / (double)k);      // -1/k is a Float64 in the reference, rounded by the store into the Float32 column; k == 0: -Inf
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < len; p += (int64_t)gridDim.x * 256) {
    int64_t d = p - first_new; if (d < 0) d += cap;
    const bool fresh = all_new || d < n_new;
    r[p] = (!fresh && ii[p] <= mx - dN) ? rold : 0.f;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------------
#define OG_STEP_SMALL 1792      // per step: info row 256 B | stats 256 B | sum-of-squares partials 768 B | NaN flag 256 B | spare 256 B
struct OgBufs { float* X; float* dz; float* xr; OgSrc* tab; double* rpart; ChainHead hd{OG_STEP_SMALL / 4}; };      // hd: a row is the first 256 B of a step's small region
static int32_t og_check(crux_ctx* c, crux_mlp* D, crux_buffer* const* srcs, int32_t K, int64_t Bd, crux_buffer* batch, const char* who) {
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  if (K < 2) return crux_fail(c, CRUX_EINVAL, "%s: %d sources; the demonstrations and the solver's buffer are the first two", who, K);
  if (K > OFFGAIL_MAXK) return crux_fail(c, CRUX_EUNSUP, "%s: %d sources, at most %d", who, K, OFFGAIL_MAXK);
  if (Bd < 1) return crux_fail(c, CRUX_EINVAL, "%s: batch %lld out of range", who, (long long)Bd);
  if ((int64_t)K * Bd > (1 << 20)) return crux_fail(c, CRUX_EUNSUP, "%s: %d x %lld columns, more than the 2^20 one forward pass takes", who, K, (long long)Bd);
  const crux_buffer* f = srcs ? srcs[0] : batch;
  for (int k = 0; srcs && k < K; ++k) {
    const crux_buffer* b = srcs[k];
    if (!b) return crux_fail(c, CRUX_EINVAL, "%s: source %d is NULL", who, k);
    if (b->obs_dim != f->obs_dim || b->act_dim != f->act_dim || b->act_kind != f->act_kind) return crux_fail(c, CRUX_EINVAL, "%s: source %d differs in obs_dim, act_dim or action kind", who, k);
    if (b->elements < 1) return crux_fail(c, CRUX_EINVAL, "%s: source %d is empty", who, k);
    if (b->prioritized) return crux_fail(c, CRUX_EUNSUP, "%s: source %d is prioritized (prioritized_sample! and its :weight rewrite are not implemented here)", who, k);
  }
  if (batch && (batch->obs_dim != f->obs_dim || batch->act_dim != f->act_dim || batch->act_kind != f->act_kind))
    return crux_fail(c, CRUX_EINVAL, "%s: the staging batch differs from the sources in obs_dim, act_dim or action kind", who);
  if (batch && batch->elements < 1) return crux_fail(c, CRUX_EINVAL, "%s: empty staging batch", who);
  const NetDesc& nd = D->nd; const int sd = f->obs_dim + f->act_dim;
  if (nd.L < 1 || nd.dims[0] != sd || nd.dims[nd.L] != K || nd.n_extra != 0) return crux_fail(c, CRUX_EINVAL, "%s: the discriminator must map vcat(s, a) (%d) -> %d classes", who, sd, K);
  return CRUX_OK;
}
// one scratch block for E steps over NC columns and a reward rewrite over B columns (0: none); the shared status word and the small regions are zeroed
static int32_t og_prepare(crux_ctx* c, int sd, int K, int64_t NC, int64_t B, int E, OgBufs& ob, const char* who) {
  const size_t bytes = Carve::span<float>((size_t)sd * NC) + Carve::span<float>((size_t)K * NC) + Carve::span<float>((size_t)sd * B) + Carve::span<OgSrc>(OFFGAIL_MAXK) +
                       Carve::span<double>(OFFGAIL_RBLOCKS) + ob.hd.bytes(E) + 256;
  Carve cv{(char*)crux_scratch(c, bytes), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch (%zu bytes)", who, bytes);
  ob.X = cv.take<float>((size_t)sd * NC); ob.dz = cv.take<float>((size_t)K * NC); ob.xr = cv.take<float>((size_t)sd * B); ob.tab = cv.take<OgSrc>(OFFGAIL_MAXK);
  ob.rpart = cv.take<double>(OFFGAIL_RBLOCKS); ob.hd.carve(cv, E);
  HIPCHK(c, hipMemsetAsync(ob.rpart, 0, Carve::span<double>(OFFGAIL_RBLOCKS) + ob.hd.extent, c->stream));      // the reward's partials sit right in front of the head
  return CRUX_OK;
}
static int32_t og_upload_sources(crux_ctx* c, crux_buffer* const* srcs, int K, OgSrc* h_tab, const OgBufs& ob) {
  for (int k = 0; k < K; ++k) { h_tab[k].s = (const float*)srcs[k]->col[CRUX_COL_S]; h_tab[k].a = srcs[k]->col[CRUX_COL_A]; h_tab[k].n = srcs[k]->elements; }
  HIPCHK(c, hipMemcpyAsync(ob.tab, h_tab, sizeof(OgSrc) * (size_t)K, hipMemcpyHostToDevice, c->stream));
  return CRUX_OK;
}
struct OgStep { float* dinfo; double* stats; double* ssq; int32_t* nanflag; };
static OgStep og_step(const OgBufs& ob, int e) {
  Carve sv{(char*)ob.hd.rows + (size_t)e * OG_STEP_SMALL, 0}; OgStep t;
  t.dinfo = sv.take<float>(CRUX_INFO_N); t.stats = sv.take<double>(8); t.ssq = sv.take<double>(2 + SUMSQ_BLOCKS); t.nanflag = sv.take<int32_t>(1); return t;
}
// step e of a call, enqueued only
static int32_t og_enqueue_step(crux_mlp* D, const crux_buffer* f, int K, int64_t Bd, uint64_t seed, uint64_t counter, const OgBufs& ob, int e) {
  crux_ctx* c = D->ctx; const int od = f->obs_dim, ad = f->act_dim; const int64_t NC = (int64_t)K * Bd;
  const OgStep t = og_step(ob, e); float* dinfo = t.dinfo; double* stats = t.stats; double* ssq = t.ssq; int32_t* nanflag = t.nanflag;
  hipLaunchKernelGGL(k_offgail_gather, dim3(nblk(Bd), (unsigned)K), dim3(256), 0, c->stream, (const OgSrc*)ob.tab, f->act_kind == CRUX_ACTION_DISCRETE ? 1 : 0, od, ad, Bd, seed, counter, ob.X, nanflag);
  int32_t rc = crux_launch_check(c, "k_offgail_gather"); if (rc) return rc;
  rc = crux_dense_forward(D, ob.X, NC, c->stream); if (rc) return rc;
  hipLaunchKernelGGL(k_offgail_ce_head, dim3(1), dim3(256), 0, c->stream, (const float*)crux_dense_act(D, D->nd.L), K, Bd, NC, (const int32_t*)nanflag, ob.dz, stats);
  rc = crux_launch_check(c, "k_offgail_ce_head"); if (rc) return rc;
  Sumsq2Fix fx{};
  rc = crux_dense_backward(D, ob.X, NC, ob.dz, 1.0f, true, nullptr, c->stream, &fx, 0); if (rc) return rc;
  crux_launch<Sumsq2Op>(SUMSQ_BLOCKS, 256, c->stream, D->g, (int64_t)D->nd.n_params, (float*)nullptr, (int64_t)0, ssq, fx);
  hipLaunchKernelGGL(k_offgail_info, dim3(1), dim3(1), 0, c->stream, (const double*)stats, (const double*)ssq, NC, dinfo);
  rc = crux_launch_check(c, "k_offgail_info"); if (rc) return rc;
  return adam_gated(D, ssq, ob.hd.status);
}
static int32_t og_enqueue_reward(crux_mlp* D, crux_buffer* b, int K, const OgBufs& ob, const int32_t* status) {
  crux_ctx* c = D->ctx; const int od = b->obs_dim, ad = b->act_dim, sd = od + ad; const int64_t B = b->elements;
  hipLaunchKernelGGL(k_offgail_concat, dim3(nblk(B * sd)), dim3(256), 0, c->stream, (const float*)b->col[CRUX_COL_S], (const void*)b->col[CRUX_COL_A], b->act_kind == CRUX_ACTION_DISCRETE ? 1 : 0, od, ad, B, ob.xr);
  int32_t rc = crux_dense_forward(D, ob.xr, B, c->stream); if (rc) return rc;
  hipLaunchKernelGGL(k_offgail_reward, dim3(OFFGAIL_RBLOCKS), dim3(256), 0, c->stream, (const float*)crux_dense_act(D, D->nd.L), K, B, K > 2 ? (float)(-1.0 / (double)(K - 2)) : 0.f, status,
                     (float*)b->col[CRUX_COL_R], ob.rpart);
  return crux_launch_check(c, "k_offgail_reward");
}

extern "C" {

int32_t crux_offgail_gather(crux_buffer* const* sources, int32_t K, int64_t Bd, uint64_t seed, uint64_t counter, float* d_X) {
  if (!sources || K < 1 || !sources[0] || !d_X) return CRUX_EINVAL;
  crux_ctx* c = sources[0]->ctx; const char* who = "offgail_gather"; const crux_buffer* f = sources[0];
  if (K > OFFGAIL_MAXK || Bd < 1 || (int64_t)K * Bd > (1 << 20)) return crux_fail(c, CRUX_EINVAL, "%s: K = %d, Bd = %lld out of range", who, K, (long long)Bd);
  for (int k = 0; k < K; ++k) if (!sources[k] || sources[k]->elements < 1 || sources[k]->obs_dim != f->obs_dim || sources[k]->act_dim != f->act_dim || sources[k]->act_kind != f->act_kind)
    return crux_fail(c, CRUX_EINVAL, "%s: source %d is empty or differs in shape", who, k);
  OgBufs ob{}; int32_t rc = og_prepare(c, 0, 0, 0, 0, 1, ob, who); if (rc) return rc;
  OgSrc* h = (OgSrc*)crux_pinned(c, sizeof(OgSrc) * OFFGAIL_MAXK); if (!h) return crux_fail(c, CRUX_ENOMEM, "%s: pinned staging", who);
  rc = og_upload_sources(c, sources, K, h, ob); if (rc) return rc;
  hipLaunchKernelGGL(k_offgail_gather, dim3(nblk(Bd), (unsigned)K), dim3(256), 0, c->stream, (const OgSrc*)ob.tab, f->act_kind == CRUX_ACTION_DISCRETE ? 1 : 0, f->obs_dim, f->act_dim, Bd, seed, counter,
                     d_X, og_step(ob, 0).nanflag);
  rc = crux_launch_check(c, "k_offgail_gather"); if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CRUX_OK;
}

// the steps of one call and (batch != NULL) the reward rewrite, one host synchronisation at the end
static int32_t og_run(crux_mlp* D, crux_buffer* const* sources, int32_t K, int64_t Bd, int32_t E, crux_buffer* batch, uint64_t seed, uint64_t counter0, float* info_out, const char* who) {
  crux_ctx* c = D->ctx; const crux_buffer* f = sources[0]; const int sd = f->obs_dim + f->act_dim; const int64_t NC = (int64_t)K * Bd, B = batch ? batch->elements : 0;
  if (!D->has_adam) return crux_fail(c, CRUX_EINVAL, "train!: crux_adam_init was not called on this handle");
  int32_t rc = ensure_ws(D, NC > B ? NC : B); if (rc) return rc;      // the workspace must not be re-allocated between the steps and the reward's forward pass
  OgBufs ob{}; rc = og_prepare(c, sd, K, NC, B, E, ob, who); if (rc) return rc;
  const size_t hb = sizeof(OgSrc) * OFFGAIL_MAXK, rb = ob.hd.run_bytes(E);
  char* h = (char*)crux_pinned(c, hb + rb); if (!h) return crux_fail(c, CRUX_ENOMEM, "%s: pinned staging", who);
  rc = og_upload_sources(c, sources, K, (OgSrc*)h, ob); if (rc) return rc;
  for (int e = 0; e < E; ++e) { rc = og_enqueue_step(D, f, K, Bd, seed, counter0 + (uint64_t)e, ob, e); if (rc) return rc; }
  if (batch) { rc = og_enqueue_reward(D, batch, K, ob, ob.hd.status); if (rc) return rc; }
  // the one host synchronisation, behind the source table in the same pinned block. The same info Dict goes to every train!: the last one's entries stay (training.jl:22-24)
  int32_t st; const char* hh; rc = ob.hd.fetch(c, rb, who, &st, &hh, hb); if (rc) return rc;
  const int last = chain_report(st, (const float*)(hh + 256), ob.hd.stride, E, E, false, info_out, nullptr);
  if (st == CRUX_ENAN) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20) in %s, discriminator epoch %d", who, last + 1);
  return CRUX_OK;
}

int32_t crux_offgail_d_step(crux_mlp* D, crux_buffer* const* sources, int32_t K, int64_t Bd, uint64_t seed, uint64_t counter, float* info_out) {
  if (!D || !sources) return CRUX_EINVAL;
  CRUX_NARROW_ONLY("crux_offgail_d_step", D);
  const char* who = "offgail_d_step"; int32_t rc = og_check(D->ctx, D, sources, K, Bd, nullptr, who); if (rc) return rc;
  return og_run(D, sources, K, Bd, 1, nullptr, seed, counter, info_out, who);
}

int32_t crux_offgail_round(crux_mlp* D, crux_buffer* const* sources, int32_t K, int64_t Bd, int32_t d_epochs, crux_buffer* batch, uint64_t seed, uint64_t counter0, float* info_out) {
  if (!D || !sources || !batch) return CRUX_EINVAL;
  CRUX_NARROW_ONLY("crux_offgail_round", D);
  const char* who = "GAIL_callback"; int32_t rc = og_check(D->ctx, D, sources, K, Bd, batch, who); if (rc) return rc;
  if (d_epochs < 1 || d_epochs > 4096) return crux_fail(D->ctx, CRUX_EINVAL, "%s: d_epochs = %d out of range", who, d_epochs);
  return og_run(D, sources, K, Bd, d_epochs, batch, seed, counter0, info_out, who);
}

int32_t crux_offgail_reward(crux_mlp* D, crux_buffer* batch, int32_t K, float* mean_r) {
  if (!D || !batch) return CRUX_EINVAL;
  CRUX_NARROW_ONLY("crux_offgail_reward", D);
  crux_ctx* c = D->ctx; const char* who = "offgail_reward";
  int32_t rc = og_check(c, D, nullptr, K, 1, batch, who); if (rc) return rc;
  const int64_t B = batch->elements; if (B > (1 << 20)) return crux_fail(c, CRUX_EUNSUP, "%s: %lld columns, more than the 2^20 one forward pass takes", who, (long long)B);
  OgBufs ob{}; rc = og_prepare(c, batch->obs_dim + batch->act_dim, K, 0, B, 0, ob, who); if (rc) return rc;
  rc = og_enqueue_reward(D, batch, K, ob, nullptr); if (rc) return rc;
  double* h = (double*)crux_pinned(c, sizeof(double) * OFFGAIL_RBLOCKS); if (!h) return crux_fail(c, CRUX_ENOMEM, "%s: pinned staging", who);
  HIPCHK(c, hipMemcpyAsync(h, ob.rpart, sizeof(double) * OFFGAIL_RBLOCKS, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  double s = 0; for (int k = 0; k < OFFGAIL_RBLOCKS; ++k) s += h[k];
  if (mean_r) *mean_r = (float)(s / (double)B);
  return CRUX_OK;
}

int32_t crux_adril_relabel(crux_buffer* ring, int64_t n_new, int64_t buffer_init, int64_t dN, int64_t* max_i_out, int64_t* k_out) {
  if (!ring) return CRUX_EINVAL;
  crux_ctx* c = ring->ctx; const char* who = "AdRIL_callback";
  if (crux_exec_recording(c)) return crux_fail(c, CRUX_EUNSUP, "%s: not recordable into a fused sequence", who);
  if (!has_col(ring, CRUX_COL_I)) return crux_fail(c, CRUX_EINVAL, "%s: the buffer has no :i column (AdRIL's default buffer carries [:i])", who);
  if (n_new < 0 || dN < 1) return crux_fail(c, CRUX_EINVAL, "%s: n_new = %lld, dN = %lld out of range", who, (long long)n_new, (long long)dN);
  const int64_t len = ring->elements, cap = ring->capacity;
  if (max_i_out) *max_i_out = 0; if (k_out) *k_out = 0;
  if (len < 1) return CRUX_OK;
  const bool all_new = len <= n_new; if (n_new > len) n_new = len;
  int64_t first_new = (ring->next_ind - n_new) % cap; if (first_new < 0) first_new += cap;
  Carve cv{(char*)crux_scratch(c, 1024), 0}; if (!cv.p) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  int64_t* part = cv.take<int64_t>(ADRIL_BLOCKS); int64_t* out = cv.take<int64_t>(4);
  const int64_t* ii = (const int64_t*)ring->col[CRUX_COL_I];
  hipLaunchKernelGGL(k_adril_max, dim3(ADRIL_BLOCKS), dim3(256), 0, c->stream, ii, len, part);
  const unsigned nb = nblk(len) < 1024u ? nblk(len) : 1024u;
  hipLaunchKernelGGL(k_adril_relabel, dim3(nb), dim3(256), 0, c->stream, ii, (float*)ring->col[CRUX_COL_R], len, cap, first_new, n_new, all_new ? 1 : 0, buffer_init, dN, (const int64_t*)part, out);
  int32_t rc = crux_launch_check(c, "k_adril_relabel"); if (rc) return rc;
  int64_t* h = (int64_t*)crux_pinned(c, 32); if (!h) return crux_fail(c, CRUX_ENOMEM, "%s: pinned staging", who);
  HIPCHK(c, hipMemcpyAsync(h, out, 24, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  if (max_i_out) *max_i_out = h[0]; if (k_out) *k_out = h[1];
  if (h[2]) return crux_fail(c, CRUX_EINVAL, "%s: InexactError: Int((%lld - %lld) / %lld) (AdRIL.jl:44); the buffer is unchanged", who, (long long)h[0], (long long)buffer_init, (long long)dN);
  return CRUX_OK;
}

}  // extern "C"
