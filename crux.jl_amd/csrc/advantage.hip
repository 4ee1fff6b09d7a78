// advantage.hip -- fill_gae! / fill_returns! / whiten on device columns.
// Reference: src/sampler.jl:255-281 (GAE + returns), src/utils.jl:41-42 (whiten), episodes() src/experience_buffer.jl:194-212.
#include "common.h"
#include <vector>

int32_t crux_mlp_forward_impl(crux_mlp* net, const float* d_x, int64_t B, float* d_y, const float* params_override);

// A block of rows to scan: block row k lives at physical row (first + k) mod cap of the ring, and rows [e*seg, (e+1)*seg) of the block belong to environment e:
// no episode crosses that boundary. A run ends on an :episode_end row, on the last row of its segment and on the block's last row. close_last: such a trailing
// run is an episode even without :episode_end (episodes(d) closes a trailing episode at length(d), experience_buffer.jl:207-211; steps!(reset=true) sets the flag
// itself); otherwise its rows keep what mdp_data put into the reference's fresh `data` block, which terminate_episode! never reached (sampler.jl:53-57,140-148).
// The whole buffer is the physical rows {0, elements, capacity} as one closed segment, wherever next_ind stands: phys(k) == k.
struct ScanRange {
  int64_t first, n, cap, seg; int close_last;
  __device__ __forceinline__ int64_t phys(int64_t k) const { const int64_t q = first + k; return q >= cap ? q - cap : q; }
  // row i ends a run: lo = the first row of its segment, open = the run trails the segment and stays as the fresh block left it
  __device__ __forceinline__ bool ends_run(const uint8_t* __restrict__ ee, int64_t i, int64_t& lo, bool& open) const {
    const bool closed = ee[phys(i)];
    if (!(closed || i == n - 1 || (i + 1) % seg == 0)) return false;
    lo = (i / seg) * seg; open = !closed && !close_last; return true;
  }
};
__host__ __device__ __forceinline__ ScanRange scan_range(int64_t first, int64_t n, int64_t cap, int64_t seg, int close_last) {      // seg <= 0: one segment of n rows
  return ScanRange{first, n, cap, seg > 0 ? seg : n, close_last ? 1 : 0};
}
__host__ __device__ __forceinline__ ScanRange scan_whole(int64_t n, int64_t cap) { return scan_range(0, n, cap, 0, 1); }

// One thread per episode: a thread sitting on a row that ends a run walks the run backwards.
// The recurrence is evaluated sequentially in Float32 with the reference's association
//   A = ((c*A + r) + ((1f0 - done)*gamma)*Vsp) - Vs        (sampler.jl:269)
//   R = r + gamma*R                                        (sampler.jl:278)
// so results are bit-identical to the scalar loop given the same V(s), V(sp). Vs / Vsp are indexed by the block row; an open trailing run gets 0.
__device__ __forceinline__ void gae_returns_body(const float* __restrict__ r, const uint8_t* __restrict__ done, const uint8_t* __restrict__ ee,
                              const float* __restrict__ Vs, const float* __restrict__ Vsp, float lambda, float gamma, const ScanRange g,
                              float* __restrict__ adv, float* __restrict__ ret, int32_t* __restrict__ nan_flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t k0; bool open;
    if (!g.ends_run(ee, i, k0, open)) continue;
    if (open) {
      for (int64_t k = i; k >= k0 && !ee[g.phys(k)]; --k) { if (adv) adv[g.phys(k)] = 0.f; if (ret) ret[g.phys(k)] = 0.f; }
      continue;
    }
    float A = 0.f, R = 0.f; const float c = __fmul_rn(lambda, gamma);
    bool bad = false;
    for (int64_t k = i; k >= k0 && (k == i || !ee[g.phys(k)]); --k) {
      const int64_t q = g.phys(k);
      const float rk = r[q];
      if (adv) {
        const float t2 = __fadd_rn(__fmul_rn(c, A), rk);
        const float t3 = __fmul_rn(__fmul_rn(__fsub_rn(1.f, done[q] ? 1.f : 0.f), gamma), Vsp[k]);
        A = __fsub_rn(__fadd_rn(t2, t3), Vs[k]);
        adv[q] = A; bad |= isnan(A);
      }
      if (ret) { R = __fadd_rn(rk, __fmul_rn(gamma, R)); ret[q] = R; }
    }
    if (bad) atomicOr(nan_flag, 1);
  }
}
__global__ void k_gae_returns(const float* __restrict__ r, const uint8_t* __restrict__ done, const uint8_t* __restrict__ ee,
                              const float* __restrict__ Vs, const float* __restrict__ Vsp, float lambda, float gamma, const ScanRange g,
                              float* __restrict__ adv, float* __restrict__ ret, int32_t* __restrict__ nan_flag) {
  gae_returns_body(r, done, ee, Vs, Vsp, lambda, gamma, g, adv, ret, nan_flag);
}
struct GaeJob { const float* r; const uint8_t* done; const uint8_t* ee; const float* Vs; const float* Vsp; float* adv; float* ret; int32_t* flag; };
__global__ void k_gae_returns_multi(const GaeJob* __restrict__ jobs, float lambda, float gamma, int64_t n) {     // grid.y = buffer, each scanned whole
  const GaeJob j = jobs[blockIdx.y];
  gae_returns_body(j.r, j.done, j.ee, j.Vs, j.Vsp, lambda, gamma, scan_whole(n, n), j.adv, j.ret, j.flag);
}

// whiten(v) = (v .- mean(v)) ./ std(v) (utils.jl:41-42) with Julia's own Float32 reductions: Statistics.mean = sum(A) / length(A), Statistics.std = sqrt(centralize_sumabs2(A, m) / (n - 1)),
// both through Base.mapreduce_impl's pairwise scheme (reduce.jl; pairwise_blocksize = 1024): a range of at most 1024 elements is summed from the left, a longer one is split at
// ifirst + (ilast - ifirst) >> 1 and the halves are added. One block: thread 0 walks the recursion once to list the leaves, thread i sums leaf i from the left, thread 0 walks it
// again to add the leaf sums in the tree's order -- the oracle's orc_jl_mean_f32 / orc_jl_std_f32 bit for bit (round 5; the Float64 tree sums before agreed with the oracle, not with Julia).
#define JLW_MAXLEAF 4096        // leaves of one reduction: n up to ~2 M elements (an on-policy buffer); larger columns are refused by the host
struct JlFrame { int64_t a, b; float v1; int st; };
__device__ __forceinline__ float jlw_term(float x, bool centred, float m) { if (!centred) return x; const float d = __fsub_rn(x, m); return __fmul_rn(d, d); }
__device__ float jlw_reduce(const float* __restrict__ v, int64_t n, bool centred, float m, int32_t* leaf_lo, float* leaf_sum, int* n_leaf) {      // leaves are contiguous: leaf q = [leaf_lo[q], leaf_lo[q + 1])
  const int tid = threadIdx.x;
  __shared__ JlFrame stk[48];      // the recursion stack of thread 0 (its only user): LDS, not 1 152 bytes of private memory per thread of the launch
  if (tid == 0) {      // the leaves of mapreduce_impl(f, +, A, 1, n, 1024) in the order the recursion visits them
    int sp = 0, nl = 0; stk[sp++] = JlFrame{0, n - 1, 0.f, 0};
    while (sp) { JlFrame f = stk[sp - 1];
      if (f.b - f.a < 1024) { leaf_lo[nl] = (int32_t)f.a; ++nl; --sp; continue; }
      const int64_t mid = f.a + ((f.b - f.a) >> 1);
      if (f.st == 0) { stk[sp - 1].st = 1; stk[sp++] = JlFrame{f.a, mid, 0.f, 0}; continue; }
      if (f.st == 1) { stk[sp - 1].st = 2; stk[sp++] = JlFrame{mid + 1, f.b, 0.f, 0}; continue; }
      --sp; }
    leaf_lo[nl] = (int32_t)n; *n_leaf = nl; }
  __syncthreads();
  const int nl = *n_leaf;
  for (int q = tid; q < nl; q += 1024) { const int64_t lo = leaf_lo[q], hi = (int64_t)leaf_lo[q + 1] - 1;      // v = f(a1) + f(a2); v += f(a3); ... (reduce.jl, the sequential portion)
    float acc = jlw_term(v[lo], centred, m);
    int64_t i = lo + 1;
    for (; i + 15 <= hi; i += 16) { float x[16];      // 16 loads in flight, then the 16 additions in order (the sum itself is a serial chain; one load per addition made it a memory round trip each)
#pragma unroll
      for (int k = 0; k < 16; ++k) x[k] = v[i + k];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc = __fadd_rn(acc, jlw_term(x[k], centred, m)); }
    for (; i <= hi; ++i) acc = __fadd_rn(acc, jlw_term(v[i], centred, m));
    leaf_sum[q] = acc; }
  __syncthreads();
  __shared__ float result;
  if (tid == 0) {      // op(v1, v2) up the same tree
    int sp = 0, nx = 0; float ret = 0.f; stk[sp++] = JlFrame{0, n - 1, 0.f, 0};
    while (sp) { JlFrame f = stk[sp - 1];
      if (f.b - f.a < 1024) { ret = leaf_sum[nx++]; --sp; continue; }
      const int64_t mid = f.a + ((f.b - f.a) >> 1);
      if (f.st == 0) { stk[sp - 1].st = 1; stk[sp++] = JlFrame{f.a, mid, 0.f, 0}; continue; }
      if (f.st == 1) { stk[sp - 1].v1 = ret; stk[sp - 1].st = 2; stk[sp++] = JlFrame{mid + 1, f.b, 0.f, 0}; continue; }
      ret = __fadd_rn(f.v1, ret); --sp; }
    result = ret; }
  __syncthreads();
  const float r = result;
  __syncthreads();
  return r;
}
__device__ __forceinline__ void whiten_block(float* __restrict__ v, int64_t n) {
  __shared__ int32_t leaf_lo[JLW_MAXLEAF + 1];
  __shared__ float leaf_sum[JLW_MAXLEAF];
  __shared__ int n_leaf;
  const float mean = __fdiv_rn(jlw_reduce(v, n, false, 0.f, leaf_lo, leaf_sum, &n_leaf), (float)n);                 // sum(A) / length(A)
  const float sd = sqrtf(__fdiv_rn(jlw_reduce(v, n, true, mean, leaf_lo, leaf_sum, &n_leaf), (float)(n - 1)));        // sqrt(centralize_sumabs2(A, m) / (n - 1))
  for (int64_t i = threadIdx.x; i < n; i += 1024) v[i] = __fdiv_rn(__fsub_rn(v[i], mean), sd);
}
__global__ __launch_bounds__(1024) void k_whiten(float* __restrict__ v, int64_t n) { whiten_block(v, n); }
__global__ __launch_bounds__(1024) void k_whiten_multi(float* const* __restrict__ vs, int64_t n) { whiten_block(vs[blockIdx.x], n); }
// NDA-GAIL's advantage tail (nda_gail_js.jl:51-61): the reward scan and the cost scan as one launch (grid.y = channel), GAE and returns of a channel in one pass, then
// both whitens as one launch (one block each). gate (may be NULL): nothing is written once the round's discriminator chains stopped with CRUX_ENAN.
__global__ void k_nda_gae2(const float* __restrict__ r, const float* __restrict__ cost, const uint8_t* __restrict__ done, const uint8_t* __restrict__ ee, const float* __restrict__ Vs,
                           const float* __restrict__ Vsp, const float* __restrict__ Cs, const float* __restrict__ Csp, float lambda, float gamma, int64_t n, float* __restrict__ adv,
                           float* __restrict__ ret, float* __restrict__ cadv, float* __restrict__ cret, int32_t* __restrict__ flags, const int32_t* __restrict__ gate) {
  if (gate && gate[0] == CRUX_ENAN) return;
  if (blockIdx.y == 0) gae_returns_body(r, done, ee, Vs, Vsp, lambda, gamma, scan_whole(n, n), adv, ret, flags);
  else gae_returns_body(cost, done, ee, Cs, Csp, lambda, gamma, scan_whole(n, n), cadv, cret, flags + 1);
}
__global__ __launch_bounds__(1024) void k_nda_whiten2(float* __restrict__ v0, float* __restrict__ v1, int64_t n, const int32_t* __restrict__ gate) {
  if (gate && gate[0] == CRUX_ENAN) return;
  whiten_block(blockIdx.x == 0 ? v0 : v1, n);
}

static int32_t values(crux_mlp* critic, const float* d_x, int64_t n, float* d_y) {
  return crux_mlp_forward_impl(critic, d_x, n, d_y, nullptr);   // 2 x 65536 critic evaluations = 0.14 ms per iteration with the generic forward kernel
}

// episodes!-style evaluation (sampler.jl:175-251) over an env-major rollout block: the FIRST episode of every environment.
// undiscounted_return = sum(r) (:203-213), discounted_return = reverse recursion r + gamma*R in Float32 (:223-229), length.
__global__ void k_first_episode_metrics(const float* __restrict__ r, const uint8_t* __restrict__ ee, int n_envs, int64_t T, float gamma,
                                        float* __restrict__ und, float* __restrict__ dis, int64_t* __restrict__ len, uint8_t* __restrict__ complete) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x; if (e >= n_envs) return;
  const int64_t base = (int64_t)e * T; int64_t stop = -1;
  for (int64_t t = 0; t < T; ++t) if (ee[base + t]) { stop = t; break; }
  complete[e] = stop >= 0 ? 1 : 0;
  if (stop < 0) stop = T - 1;
  float u = 0.f, d = 0.f;
  for (int64_t t = 0; t <= stop; ++t) u = __fadd_rn(u, r[base + t]);
  for (int64_t t = stop; t >= 0; --t) d = __fadd_rn(r[base + t], __fmul_rn(gamma, d));
  und[e] = u; dis[e] = d; len[e] = stop + 1;
}

// a Float32 one-row column that exists (fill_gae!/fill_returns! `source=` / `target=` keywords, sampler.jl:65-66,255,275)
static bool f32_scalar_col(const crux_buffer* b, int k) { return (k == CRUX_COL_R || has_col(b, k)) && col_rows(b, k) == 1 && col_elem(b, k) == 4; }

// ---- the scan driver: fill_gae!(data, ep, V, lambda, gamma) / fill_returns!(data, ep, gamma) on a block of rows -------------------------------------------------------
// everything that can refuse a scan, before anything is enqueued (critic: NULL for fill_returns!)
static int32_t scan_check(const crux_buffer* b, const crux_mlp* critic, int32_t source, int32_t target, const ScanRange& g, const char* who) {
  crux_ctx* c = b->ctx;
  if (!f32_scalar_col(b, source) || !f32_scalar_col(b, target)) return crux_fail(c, CRUX_EINVAL, "%s: buffer lacks the source / target column (%d -> %d)", who, source, target);
  if (critic && (critic->nd.dims[critic->nd.L] != 1 || critic->nd.dims[0] != b->obs_dim)) return crux_fail(c, CRUX_EINVAL, "%s: critic must map obs(%d) -> 1 (@assert length(Vs) == 1)", who, b->obs_dim);
  if (g.first < 0 || g.first >= g.cap || g.n < 0 || g.n > g.cap) return crux_fail(c, CRUX_EINVAL, "%s: rows [%lld, +%lld) outside the ring of %lld", who, (long long)g.first, (long long)g.n, (long long)g.cap);
  return CRUX_OK;
}
// V(s), V(sp) of the block's rows in block order: the rows up to the ring's end, then the wrapped ones
static int32_t block_values(crux_mlp* critic, const crux_buffer* b, const ScanRange& g, float* Vs, float* Vsp) {
  const int64_t n1 = g.first + g.n <= g.cap ? g.n : g.cap - g.first, n2 = g.n - n1; const int od = b->obs_dim;
  int32_t rc = values(critic, (const float*)b->col[CRUX_COL_S] + g.first * od, n1, Vs); if (rc) return rc;
  rc = values(critic, (const float*)b->col[CRUX_COL_SP] + g.first * od, n1, Vsp); if (rc) return rc;
  if (n2 > 0) { rc = values(critic, (const float*)b->col[CRUX_COL_S], n2, Vs + n1); if (rc) return rc;
    rc = values(critic, (const float*)b->col[CRUX_COL_SP], n2, Vsp + n1); if (rc) return rc; }
  return CRUX_OK;
}
// the scan's one launch; adv_target / ret_target: -1 = not filled
static void scan_enqueue(const crux_buffer* b, float lambda, float gamma, const ScanRange& g, int32_t source, int32_t adv_target, int32_t ret_target, const float* Vs, const float* Vsp, int32_t* flag) {
  hipLaunchKernelGGL(k_gae_returns, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, b->ctx->stream, (const float*)b->col[source], (const uint8_t*)b->col[CRUX_COL_DONE],
                     (const uint8_t*)b->col[CRUX_COL_EPISODE_END], Vs, Vsp, lambda, gamma, g, adv_target >= 0 ? (float*)b->col[adv_target] : (float*)nullptr,
                     ret_target >= 0 ? (float*)b->col[ret_target] : (float*)nullptr, flag);
}
static int32_t scan_flag(crux_ctx* c, const int32_t* flag) {      // the scan's one host synchronisation
  int32_t h = 0;
  HIPCHK(c, hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return h ? crux_fail(c, CRUX_ENAN, "fill_gae!: NaN advantage (@assert !isnan(A))") : CRUX_OK;
}
// critic: source -> target is an advantage, its NaN flag is read back; NULL: a return, enqueued only (the flag word is a valid address and nothing more)
static int32_t scan_fill(crux_buffer* b, crux_mlp* critic, float lambda, float gamma, const ScanRange g, int32_t source, int32_t target) {
  crux_ctx* c = b->ctx; const char* who = critic ? "fill_gae!" : "fill_returns!";
  int32_t rc = scan_check(b, critic, source, target, g, who); if (rc) return rc;
  if (g.n == 0) return CRUX_OK;
  const size_t vb = critic ? Carve::span<float>((size_t)g.n) : 0;
  char* sc = (char*)crux_scratch(c, 2 * vb + 256);
  if (!sc) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  float* Vs = (float*)sc; float* Vsp = (float*)(sc + vb); int32_t* flag = (int32_t*)(sc + 2 * vb);
  if (critic) {
    HIPCHK(c, hipMemsetAsync(flag, 0, 4, c->stream));
    crux_prof_begin(c, CRUX_PROF_VALUES);
    rc = block_values(critic, b, g, Vs, Vsp); if (rc) return rc;
    crux_prof_end(c, CRUX_PROF_VALUES);
  }
  crux_prof_begin(c, CRUX_PROF_GAE);
  scan_enqueue(b, lambda, gamma, g, source, critic ? target : -1, critic ? -1 : target, critic ? Vs : nullptr, critic ? Vsp : nullptr, flag);
  crux_prof_end(c, CRUX_PROF_GAE);
  rc = crux_launch_check(c, "k_gae_returns"); if (rc) return rc;
  return critic ? scan_flag(c, flag) : CRUX_OK;
}
static ScanRange whole_buffer(const crux_buffer* b) { return scan_whole(b->elements, b->capacity); }

// what stands between a column and whiten_block: it is no 1 x N Float32 column, holds fewer than 2 elements, or more than the pairwise reduction's leaf tables take
enum { WHITEN_COLUMN = 1, WHITEN_FEW = 2, WHITEN_MANY = 4 };
static int whiten_unfit(const crux_buffer* b, int key) {
  return (has_col(b, key) && col_elem(b, key) == 4 && col_rows(b, key) == 1 ? 0 : WHITEN_COLUMN) | (b->elements < 2 ? WHITEN_FEW : 0) | (b->elements > (int64_t)JLW_MAXLEAF * 512 ? WHITEN_MANY : 0);
}

extern "C" {

int32_t crux_first_episode_metrics(crux_buffer* b, int32_t n_envs, int64_t T, float gamma, float* undisc, float* disc, int64_t* length, uint8_t* complete) {
  if (!b || n_envs < 1 || T < 1) return CRUX_EINVAL;
  crux_ctx* c = b->ctx;
  if ((int64_t)n_envs * T != b->elements || b->next_ind != (b->elements % b->capacity)) return crux_fail(c, CRUX_EINVAL, "episode metrics: buffer must hold exactly one %d x %lld env-major rollout block", n_envs, (long long)T);
  const size_t nb = (size_t)n_envs;
  char* sc = (char*)crux_scratch(c, nb * 17 + 1024); if (!sc) return crux_fail(c, CRUX_ENOMEM, "episode metrics: scratch");
  int64_t* d_len = (int64_t*)sc; float* d_u = (float*)(sc + 8 * nb); float* d_d = d_u + nb; uint8_t* d_c = (uint8_t*)(d_d + nb);
  hipLaunchKernelGGL(k_first_episode_metrics, dim3((unsigned)((n_envs + 63) / 64)), dim3(64), 0, c->stream, (const float*)b->col[CRUX_COL_R], (const uint8_t*)b->col[CRUX_COL_EPISODE_END],
                     n_envs, T, gamma, d_u, d_d, d_len, d_c);
  int32_t rc = crux_launch_check(c, "k_first_episode_metrics"); if (rc) return rc;
  if (undisc) HIPCHK(c, hipMemcpyAsync(undisc, d_u, 4 * nb, hipMemcpyDeviceToHost, c->stream));
  if (disc) HIPCHK(c, hipMemcpyAsync(disc, d_d, 4 * nb, hipMemcpyDeviceToHost, c->stream));
  if (length) HIPCHK(c, hipMemcpyAsync(length, d_len, 8 * nb, hipMemcpyDeviceToHost, c->stream));
  if (complete) HIPCHK(c, hipMemcpyAsync(complete, d_c, nb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CRUX_OK;
}

// The whole-buffer forms scan the physical rows 0 .. length(b)-1; the _rows forms scan what terminate_episode! applies fill_gae! / fill_returns! to: the block a steps!
// call just produced (sampler.jl:53-57,140-148), on the ring rows [first_row, first_row + n_rows) mod capacity that it was pushed to.
int32_t crux_fill_gae_keys(crux_buffer* b, crux_mlp* critic, float lambda, float gamma, int32_t source, int32_t target) { CRUX_PLAIN_ONLY("crux_fill_gae_keys", critic);
  if (!b || !critic) return CRUX_EINVAL;
  return scan_fill(b, critic, lambda, gamma, whole_buffer(b), source, target);
}
int32_t crux_fill_gae(crux_buffer* b, crux_mlp* critic, float lambda, float gamma) { CRUX_PLAIN_ONLY("crux_fill_gae", critic); return crux_fill_gae_keys(b, critic, lambda, gamma, CRUX_COL_R, CRUX_COL_ADVANTAGE); }
int32_t crux_fill_gae_rows_keys(crux_buffer* b, crux_mlp* critic, float lambda, float gamma, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last, int32_t source, int32_t target) { CRUX_PLAIN_ONLY("crux_fill_gae_rows_keys", critic);
  if (!b || !critic) return CRUX_EINVAL;
  return scan_fill(b, critic, lambda, gamma, scan_range(first_row, n_rows, b->capacity, rows_per_env, close_last), source, target);
}
int32_t crux_fill_gae_rows(crux_buffer* b, crux_mlp* critic, float lambda, float gamma, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last) { CRUX_PLAIN_ONLY("crux_fill_gae_rows", critic); return crux_fill_gae_rows_keys(b, critic, lambda, gamma, first_row, n_rows, rows_per_env, close_last, CRUX_COL_R, CRUX_COL_ADVANTAGE); }
int32_t crux_fill_returns_keys(crux_buffer* b, float gamma, int32_t source, int32_t target) {
  if (!b) return CRUX_EINVAL;
  return scan_fill(b, nullptr, 0.f, gamma, whole_buffer(b), source, target);
}
int32_t crux_fill_returns(crux_buffer* b, float gamma) { return crux_fill_returns_keys(b, gamma, CRUX_COL_R, CRUX_COL_RETURN); }
int32_t crux_fill_returns_rows_keys(crux_buffer* b, float gamma, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last, int32_t source, int32_t target) {
  if (!b) return CRUX_EINVAL;
  return scan_fill(b, nullptr, 0.f, gamma, scan_range(first_row, n_rows, b->capacity, rows_per_env, close_last), source, target);
}
int32_t crux_fill_returns_rows(crux_buffer* b, float gamma, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last) { return crux_fill_returns_rows_keys(b, gamma, first_row, n_rows, rows_per_env, close_last, CRUX_COL_R, CRUX_COL_RETURN); }

// fill_gae! + fill_returns! for n buffers (the tail of a batched rollout): everything is enqueued, ONE host synchronisation reads the n NaN flags
int32_t crux_fill_gae_multi(int32_t n, crux_buffer* const* bufs, crux_mlp* const* critics, float lambda, float gamma, int32_t with_returns) {
  if (n < 1 || !bufs || !critics) return CRUX_EINVAL;
  for (int i = 0; i < n; ++i) CRUX_PLAIN_ONLY("crux_fill_gae_multi", critics[i]);
  crux_ctx* c = bufs[0]->ctx; size_t vb = 0;
  for (int i = 0; i < n; ++i) {
    crux_buffer* b = bufs[i]; crux_mlp* critic = critics[i]; if (!b || !critic) return CRUX_EINVAL;
    if (!has_col(b, CRUX_COL_ADVANTAGE)) return crux_fail(c, CRUX_EINVAL, "fill_gae!: buffer %d has no :advantage column", i);
    if (with_returns && !has_col(b, CRUX_COL_RETURN)) return crux_fail(c, CRUX_EINVAL, "fill_returns!: buffer %d has no :return column", i);
    if (critic->nd.dims[critic->nd.L] != 1 || critic->nd.dims[0] != b->obs_dim) return crux_fail(c, CRUX_EINVAL, "fill_gae!: critic must map obs(%d) -> 1 (@assert length(Vs) == 1)", b->obs_dim);
    const size_t v = ((4 * (size_t)b->elements + 255) / 256) * 256; if (v > vb) vb = v;
  }
  bool same = true;
  for (int i = 1; i < n; ++i) same = same && bufs[i]->elements == bufs[0]->elements && critics[i]->nd.n_params == critics[0]->nd.n_params && critics[i]->nd.L == critics[0]->nd.L &&
                                     memcmp(critics[i]->nd.dims, critics[0]->nd.dims, sizeof critics[0]->nd.dims) == 0 && memcmp(critics[i]->nd.acts, critics[0]->nd.acts, sizeof critics[0]->nd.acts) == 0;
  const size_t jb = (((sizeof(crux_fwd_job) * 2 + sizeof(GaeJob)) * (size_t)n) + 255) / 256 * 256, fb = (((size_t)n * 4 + 255) / 256) * 256;
  char* sc = (char*)crux_scratch(c, fb + jb + (size_t)n * 2 * vb + 256); if (!sc) return crux_fail(c, CRUX_ENOMEM, "fill_gae! (multi): scratch");
  int32_t* flags = (int32_t*)sc; char* vals = sc + fb + jb;
  HIPCHK(c, hipMemsetAsync(flags, 0, 4 * (size_t)n, c->stream));
  const int64_t m0 = bufs[0]->elements;
  if (same && m0 > 0) {     // equal shapes: 2 launches for the 2 n critic evaluations and 1 for the n scans (grid.y = buffer)
    std::vector<char> hj(jb); crux_fwd_job* fj = (crux_fwd_job*)hj.data(); GaeJob* gj = (GaeJob*)(hj.data() + sizeof(crux_fwd_job) * 2 * (size_t)n);
    for (int i = 0; i < n; ++i) { crux_buffer* b = bufs[i]; float* Vs = (float*)(vals + (size_t)i * 2 * vb); float* Vsp = (float*)(vals + (size_t)i * 2 * vb + vb);
      fj[2 * i] = {critics[i]->p, (const float*)b->col[CRUX_COL_S], Vs}; fj[2 * i + 1] = {critics[i]->p, (const float*)b->col[CRUX_COL_SP], Vsp};
      gj[i] = {(const float*)b->col[CRUX_COL_R], (const uint8_t*)b->col[CRUX_COL_DONE], (const uint8_t*)b->col[CRUX_COL_EPISODE_END], Vs, Vsp, (float*)b->col[CRUX_COL_ADVANTAGE],
               with_returns ? (float*)b->col[CRUX_COL_RETURN] : (float*)nullptr, flags + i}; }
    HIPCHK(c, hipMemcpyAsync(sc + fb, hj.data(), jb, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
    crux_prof_begin(c, CRUX_PROF_VALUES);
    int32_t rcf = crux_mlp_forward_multi_impl(c, critics[0]->nd, (const crux_fwd_job*)(sc + fb), 2 * n, m0); if (rcf) return rcf;
    crux_prof_end(c, CRUX_PROF_VALUES);
    crux_prof_begin(c, CRUX_PROF_GAE);
    hipLaunchKernelGGL(k_gae_returns_multi, dim3((unsigned)((m0 + 255) / 256), (unsigned)n), dim3(256), 0, c->stream, (const GaeJob*)(sc + fb + sizeof(crux_fwd_job) * 2 * (size_t)n), lambda, gamma, m0);
    crux_prof_end(c, CRUX_PROF_GAE);
  } else {                  // the single buffer's passes, one buffer after the other: all values, then all scans
    crux_prof_begin(c, CRUX_PROF_VALUES);
    for (int i = 0; i < n; ++i) { if (bufs[i]->elements == 0) continue;
      int32_t rc = block_values(critics[i], bufs[i], whole_buffer(bufs[i]), (float*)(vals + (size_t)i * 2 * vb), (float*)(vals + (size_t)i * 2 * vb + vb)); if (rc) return rc; }
    crux_prof_end(c, CRUX_PROF_VALUES);
    crux_prof_begin(c, CRUX_PROF_GAE);
    for (int i = 0; i < n; ++i) { if (bufs[i]->elements == 0) continue;
      scan_enqueue(bufs[i], lambda, gamma, whole_buffer(bufs[i]), CRUX_COL_R, CRUX_COL_ADVANTAGE, with_returns ? CRUX_COL_RETURN : -1, (const float*)(vals + (size_t)i * 2 * vb),
                   (const float*)(vals + (size_t)i * 2 * vb + vb), flags + i); }
    crux_prof_end(c, CRUX_PROF_GAE);
  }
  int32_t rc = crux_launch_check(c, "k_gae_returns (multi)"); if (rc) return rc;
  std::vector<int32_t> h((size_t)n);
  HIPCHK(c, hipMemcpyAsync(h.data(), flags, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) if (h[(size_t)i]) return crux_fail(c, CRUX_ENAN, "fill_gae!: NaN advantage in buffer %d (@assert !isnan(A))", i);
  return CRUX_OK;
}

int32_t crux_whiten_multi(int32_t n, crux_buffer* const* bufs, int32_t key) {
  if (n < 1 || !bufs) return CRUX_EINVAL;
  crux_ctx* c = bufs[0]->ctx; const int64_t len = bufs[0]->elements;
  if (whiten_unfit(bufs[0], key) & WHITEN_MANY) return crux_fail(c, CRUX_EUNSUP, "whiten (multi): %lld elements per buffer (the pairwise reduction is laid out for at most %d leaves)", (long long)len, JLW_MAXLEAF);      // k_whiten_multi keeps the leaf tables in LDS
  std::vector<float*> hp((size_t)n);
  for (int i = 0; i < n; ++i) { crux_buffer* b = bufs[i]; const int unfit = b ? whiten_unfit(b, key) : WHITEN_COLUMN;
    if (unfit & WHITEN_COLUMN) return crux_fail(c, CRUX_EINVAL, "whiten: column %d of buffer %d is not a 1 x N Float32 column", key, i);
    if (b->elements != len || (unfit & WHITEN_FEW)) return crux_fail(c, CRUX_EINVAL, "whiten (multi): buffers must hold the same number (>= 2) of elements");
    hp[(size_t)i] = (float*)b->col[key]; }
  float** dp = (float**)crux_scratch(c, 8 * (size_t)n + 256); if (!dp) return crux_fail(c, CRUX_ENOMEM, "whiten (multi): scratch");
  HIPCHK(c, hipMemcpyAsync(dp, hp.data(), 8 * (size_t)n, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  crux_prof_begin(c, CRUX_PROF_WHITEN);
  hipLaunchKernelGGL(k_whiten_multi, dim3((unsigned)n), dim3(1024), 0, c->stream, (float* const*)dp, len);
  crux_prof_end(c, CRUX_PROF_WHITEN);
  return crux_launch_check(c, "k_whiten_multi");
}

int32_t crux_whiten(crux_buffer* b, int32_t key) {
  if (!b) return CRUX_EINVAL;
  crux_ctx* c = b->ctx;
  const int64_t n = b->elements; const int unfit = whiten_unfit(b, key);
  if (unfit & WHITEN_COLUMN) return crux_fail(c, CRUX_EINVAL, "whiten: column %d is not a 1 x N Float32 column", key);
  if (unfit & WHITEN_FEW) return crux_fail(c, CRUX_EINVAL, "whiten: need at least 2 elements");
  if (unfit & WHITEN_MANY) return crux_fail(c, CRUX_EUNSUP, "whiten: %lld elements (the pairwise reduction is laid out for at most %d leaves)", (long long)n, JLW_MAXLEAF);
  crux_prof_begin(c, CRUX_PROF_WHITEN);
  hipLaunchKernelGGL(k_whiten, dim3(1), dim3(1024), 0, c->stream, (float*)b->col[key], n);
  crux_prof_end(c, CRUX_PROF_WHITEN);
  return crux_launch_check(c, "k_whiten");
}

}  // extern "C"

// ---- NDA-GAIL's advantage tail --------------------------------------------------------------------------------------------------------------------------------
// scratch of the enqueue-only form: V(s), V(sp), Vc(s), Vc(sp) and the two NaN flags
size_t crux_nda_adv_bytes(int64_t n) { return 4 * Carve::span<float>((size_t)n) + 256; }
int32_t crux_nda_adv_check(crux_buffer* b, crux_mlp* V, crux_mlp* Vc, const char* who) {
  crux_ctx* c = b->ctx;
  for (int k : {CRUX_COL_ADVANTAGE, CRUX_COL_RETURN, CRUX_COL_COST, CRUX_COL_COST_ADVANTAGE, CRUX_COL_COST_RETURN})
    if (!f32_scalar_col(b, k)) return crux_fail(c, CRUX_EINVAL, "%s: the buffer lacks column %d (:advantage, :return, :cost, :cost_advantage and :cost_return are needed)", who, k);
  if (V->ctx != c || Vc->ctx != c) return crux_fail(c, CRUX_EINVAL, "%s: the critics and the buffer belong to different contexts", who);
  for (crux_mlp* q : {V, Vc}) if (q->nd.L < 1 || q->nd.dims[q->nd.L] != 1 || q->nd.dims[0] != b->obs_dim)
    return crux_fail(c, CRUX_EINVAL, "%s: both critics must map obs(%d) -> 1 (@assert length(Vs) == 1)", who, b->obs_dim);
  const int unfit = whiten_unfit(b, CRUX_COL_ADVANTAGE);      // (:cost_advantage has the same shape: both passed the column test above)
  if (unfit & WHITEN_FEW) return crux_fail(c, CRUX_EINVAL, "%s: whiten needs at least 2 elements", who);
  if (unfit & WHITEN_MANY) return crux_fail(c, CRUX_EUNSUP, "%s: %lld elements (the pairwise reduction is laid out for at most %d leaves)", who, (long long)b->elements, JLW_MAXLEAF);
  return CRUX_OK;
}
// everything enqueued, nothing read: flags_out[0] / [1] are raised by a NaN reward / cost advantage (@assert !isnan(A), sampler.jl:270)
int32_t crux_nda_adv_enqueue(crux_buffer* b, crux_mlp* V, crux_mlp* Vc, float lambda, float gamma, char* sc, const int32_t* gate, int32_t** flags_out) {
  crux_ctx* c = b->ctx; const int64_t n = b->elements;
  Carve cv{sc, 0}; float* Vs = cv.take<float>((size_t)n); float* Vsp = cv.take<float>((size_t)n); float* Cs = cv.take<float>((size_t)n); float* Csp = cv.take<float>((size_t)n);
  int32_t* flags = cv.take<int32_t>(2);
  HIPCHK(c, hipMemsetAsync(flags, 0, 256, c->stream));
  crux_prof_begin(c, CRUX_PROF_VALUES);
  int32_t rc = block_values(V, b, whole_buffer(b), Vs, Vsp); if (rc) return rc;
  rc = block_values(Vc, b, whole_buffer(b), Cs, Csp); if (rc) return rc;
  crux_prof_end(c, CRUX_PROF_VALUES);
  crux_prof_begin(c, CRUX_PROF_GAE);
  hipLaunchKernelGGL(k_nda_gae2, dim3((unsigned)((n + 255) / 256), 2), dim3(256), 0, c->stream, (const float*)b->col[CRUX_COL_R], (const float*)b->col[CRUX_COL_COST], (const uint8_t*)b->col[CRUX_COL_DONE],
                     (const uint8_t*)b->col[CRUX_COL_EPISODE_END], (const float*)Vs, (const float*)Vsp, (const float*)Cs, (const float*)Csp, lambda, gamma, n, (float*)b->col[CRUX_COL_ADVANTAGE],
                     (float*)b->col[CRUX_COL_RETURN], (float*)b->col[CRUX_COL_COST_ADVANTAGE], (float*)b->col[CRUX_COL_COST_RETURN], flags, gate);
  crux_prof_end(c, CRUX_PROF_GAE);
  crux_prof_begin(c, CRUX_PROF_WHITEN);
  hipLaunchKernelGGL(k_nda_whiten2, dim3(2), dim3(1024), 0, c->stream, (float*)b->col[CRUX_COL_ADVANTAGE], (float*)b->col[CRUX_COL_COST_ADVANTAGE], n, gate);
  crux_prof_end(c, CRUX_PROF_WHITEN);
  *flags_out = flags;
  return crux_launch_check(c, "k_nda_gae2 / k_nda_whiten2");
}
extern "C" int32_t crux_nda_advantages(crux_buffer* b, crux_mlp* V, crux_mlp* Vc, float lambda, float gamma) { CRUX_PLAIN_ONLY("crux_nda_advantages", V, Vc);
  if (!b || !V || !Vc) return CRUX_EINVAL;
  crux_ctx* c = b->ctx; const char* who = "nda_advantages";
  int32_t rc = crux_nda_adv_check(b, V, Vc, who); if (rc) return rc;
  char* sc = (char*)crux_scratch(c, crux_nda_adv_bytes(b->elements)); if (!sc) return crux_fail(c, CRUX_ENOMEM, "%s: scratch", who);
  int32_t* flags = nullptr;
  rc = crux_nda_adv_enqueue(b, V, Vc, lambda, gamma, sc, nullptr, &flags); if (rc) return rc;
  int32_t* h = (int32_t*)crux_pinned(c, 8); if (!h) return crux_fail(c, CRUX_ENOMEM, "%s: pinned staging", who);
  HIPCHK(c, hipMemcpyAsync(h, flags, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[0]) return crux_fail(c, CRUX_ENAN, "fill_gae!: NaN advantage (@assert !isnan(A))");
  if (h[1]) return crux_fail(c, CRUX_ENAN, "fill_gae!: NaN cost advantage (@assert !isnan(A))");
  return CRUX_OK;
}

// ---- importance-weight columns (src/sampler.jl:58-62,108-111,283-308) ------------------------------------------------------------------------
// exp.(logpdf(pa, s, a) .- logprob): z = the nominal policy's outputs of the rows [nout x n]
__global__ void k_importance_weight(const float* __restrict__ z, int nout, const void* __restrict__ act, int act_kind, const float* __restrict__ ls, const float* __restrict__ lp, int64_t n, float* __restrict__ iw) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (j >= n) return;
  float nom;
  if (act_kind == CRUX_ACTION_DISCRETE) {      // categorical_logpdf (policies.jl:128-135): log(sum(softmax(z) .* onehot))
    const uint8_t* a = (const uint8_t*)act + j * nout; const float* zz = z + j * nout;
    float mx = zz[0]; for (int k = 1; k < nout; ++k) mx = zz[k] > mx ? zz[k] : mx;
    float sum = 0.f; for (int k = 0; k < nout; ++k) sum = __fadd_rn(sum, expf(__fsub_rn(zz[k], mx)));
    float q = 0.f; for (int k = 0; k < nout; ++k) q = __fadd_rn(q, __fmul_rn(__fdiv_rn(expf(__fsub_rn(zz[k], mx)), sum), a[k] ? 1.f : 0.f));
    nom = logf(q);
  } else {                                     // gaussian_logpdf (policies.jl:333-336)
    const float* a = (const float*)act + j * nout; const float* mu = z + j * nout; nom = 0.f;
    for (int d = 0; d < nout; ++d) { const float sg = expf(ls[d]), s2 = __fmul_rn(sg, sg), df = __fsub_rn(a[d], mu[d]);
      nom = __fadd_rn(nom, __fsub_rn(__fsub_rn(-(__fmul_rn(df, df)) / __fmul_rn(2.f, s2), 0.9189385332046727f), ls[d])); }
  }
  iw[j] = expf(__fsub_rn(nom, lp[j]));
}
// one thread per episode (the one sitting on the row that ends its run): rev walks the episode backwards, fwd forwards, cum is the product of the whole episode
__global__ void k_importance_fills(const float* __restrict__ iw, const uint8_t* __restrict__ ee, const ScanRange g, float* __restrict__ fwd, float* __restrict__ cum, float* __restrict__ rev) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t k0; bool open;
    if (!g.ends_run(ee, i, k0, open)) continue;
    int64_t start = i; while (start > k0 && !ee[g.phys(start - 1)]) --start;
    if (open) {                              // terminate_episode! never reached it, the fresh data block holds ones
      for (int64_t k = start; k <= i; ++k) { const int64_t q = g.phys(k); if (fwd) fwd[q] = 1.f; if (cum) cum[q] = 1.f; if (rev) rev[q] = 1.f; }
      continue;
    }
    float w = 1.f;
    if (rev) for (int64_t k = i; k >= start; --k) { const int64_t q = g.phys(k); w = __fmul_rn(iw[q], w); rev[q] = w; }      // :301-308
    w = 1.f;
    for (int64_t k = start; k <= i; ++k) { const int64_t q = g.phys(k); w = __fmul_rn(iw[q], w); if (fwd) fwd[q] = w; }     // :283-290
    if (cum) for (int64_t k = start; k <= i; ++k) cum[g.phys(k)] = w;                                                          // :292-299
  }
}
extern "C" int32_t crux_importance_weight_rows(crux_buffer* b, crux_mlp* nominal, int32_t head, int64_t first_row, int64_t n_rows) { CRUX_PLAIN_ONLY("crux_importance_weight_rows", nominal);
  if (!b || !nominal) return CRUX_EINVAL;
  crux_ctx* c = b->ctx;
  if (nominal->sigma_head) return crux_fail(c, CRUX_EUNSUP, "importance_weight: a two-headed Gaussian actor (logSigma network) as the nominal policy is not implemented");
  if (!has_col(b, CRUX_COL_IMPORTANCE_WEIGHT) || !has_col(b, CRUX_COL_LOGPROB)) return crux_fail(c, CRUX_EINVAL, "importance_weight: the buffer needs :importance_weight and :logprob columns");
  if (n_rows == 0) return CRUX_OK;
  if (first_row < 0 || n_rows < 0 || first_row + n_rows > b->capacity) return crux_fail(c, CRUX_EINVAL, "importance_weight: rows [%lld, %lld) outside the buffer (a wrapped range takes two calls)", (long long)first_row, (long long)(first_row + n_rows));
  const int nout = nominal->nd.dims[nominal->nd.L];
  const bool disc = b->act_kind == CRUX_ACTION_DISCRETE;
  if (nominal->nd.dims[0] != b->obs_dim || nout != b->act_dim || (disc ? head != CRUX_HEAD_CATEGORICAL : (head != CRUX_HEAD_GAUSSIAN || nominal->nd.n_extra != nout)))
    return crux_fail(c, CRUX_EINVAL, "importance_weight: the nominal policy must map obs(%d) -> %d with a %s head", b->obs_dim, b->act_dim, disc ? "categorical" : "Gaussian (logSigma extras)");
  if (nominal->squash > 0.f) return crux_fail(c, CRUX_EUNSUP, "importance_weight: SquashedGaussianPolicy nominal policies are not wired up");
  float* z = (float*)crux_scratch(c, 4 * (size_t)n_rows * nout + 256); if (!z) return crux_fail(c, CRUX_ENOMEM, "importance_weight: scratch");
  int32_t rc = crux_mlp_forward_impl(nominal, (const float*)b->col[CRUX_COL_S] + (size_t)first_row * b->obs_dim, n_rows, z, nullptr); if (rc) return rc;
  const char* act = (const char*)b->col[CRUX_COL_A] + (size_t)first_row * col_stride(b, CRUX_COL_A);
  hipLaunchKernelGGL(k_importance_weight, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, c->stream, (const float*)z, nout, (const void*)act, b->act_kind, disc ? (const float*)nullptr : (const float*)(nominal->p + nominal->nd.xoff),
                     (const float*)b->col[CRUX_COL_LOGPROB] + first_row, n_rows, (float*)b->col[CRUX_COL_IMPORTANCE_WEIGHT] + first_row);
  return crux_launch_check(c, "k_importance_weight");
}
extern "C" int32_t crux_fill_importance_weights_rows(crux_buffer* b, int64_t first_row, int64_t n_rows, int64_t rows_per_env, int32_t close_last) {
  if (!b) return CRUX_EINVAL;
  crux_ctx* c = b->ctx;
  const bool hf = has_col(b, CRUX_COL_FWD_IMPORTANCE_WEIGHT), hc = has_col(b, CRUX_COL_CUM_IMPORTANCE_WEIGHT), hr = has_col(b, CRUX_COL_REV_IMPORTANCE_WEIGHT);
  if (!hf && !hc && !hr) return CRUX_OK;
  if (!has_col(b, CRUX_COL_IMPORTANCE_WEIGHT)) return crux_fail(c, CRUX_EINVAL, "fill_*_importance_weight!: the buffer has no :importance_weight column (@assert haskey(data, :importance_weight), sampler.jl:284)");
  if (n_rows == 0) return CRUX_OK;
  if (first_row < 0 || first_row >= b->capacity || n_rows < 0 || n_rows > b->capacity) return crux_fail(c, CRUX_EINVAL, "fill_*_importance_weight!: rows out of range");
  hipLaunchKernelGGL(k_importance_fills, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, c->stream, (const float*)b->col[CRUX_COL_IMPORTANCE_WEIGHT], (const uint8_t*)b->col[CRUX_COL_EPISODE_END],
                     scan_range(first_row, n_rows, b->capacity, rows_per_env, close_last),
                     hf ? (float*)b->col[CRUX_COL_FWD_IMPORTANCE_WEIGHT] : (float*)nullptr, hc ? (float*)b->col[CRUX_COL_CUM_IMPORTANCE_WEIGHT] : (float*)nullptr, hr ? (float*)b->col[CRUX_COL_REV_IMPORTANCE_WEIGHT] : (float*)nullptr);
  return crux_launch_check(c, "k_importance_fills");
}
