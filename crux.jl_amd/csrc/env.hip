// env.hip -- vectorised Samplers: environment dynamics + policy forward + column writes in one kernel (the device bodies shared with small_solve.hip: rollout.h).
// Reference: Sampler / reset_sampler! / step! / steps! / terminate_episode! (src/sampler.jl:1-173),
// DiscreteNetwork exploration (src/policies.jl:137-142), GaussianPolicy exploration (:338-344),
// MixedPolicy (:474-494), GaussianNoiseExplorationPolicy (:510-514), LinearDecaySchedule (src/utils.jl:116-126),
// tovec whitening (src/spaces.jl:25). Environment dynamics restate gymnasium's classic_control definitions
// (the reference reaches them through POMDPGym/PyCall, src/sampler.jl:93).
#include "rollout.h"
#include "per_tree.h"

void crux_buffer_ring_advance(crux_buffer* b, int64_t N);
int32_t crux_buffer_per_on_push(crux_buffer* b, const int64_t* d_I, int64_t N);
int32_t crux_buffer_ring_ids_device(crux_buffer* b, int64_t N, int64_t* d_out);
bool crux_per_push_fused(crux_buffer* b, int64_t n, int64_t* d_ids);
bool crux_per_push_plan(crux_buffer* b, int64_t n, int* touch);
void crux_per_push_done(crux_buffer* b, int touch);

// ---- register-resident policy for the IN-64-64-OUT family ------------------------------------------------------------------------
// One wave per environment. Lane j keeps row j of W1/W2 and column j of W3 in VGPRs for the whole rollout; every lane carries an
// identical copy of the sampler state (Float64 dynamics, Philox draws and the head are evaluated redundantly), so the only
// cross-lane traffic per step is the broadcast of H1 (64 floats through LDS) and one wave reduction per output.
template <int IN, int OUT, int ACT, int KIND>
__global__ __launch_bounds__(64) void k_rollout_h64(RolloutArgs a_single, const RolloutArgs* __restrict__ multi) {
  __shared__ __attribute__((aligned(16))) float sh[64];
  // multi != NULL: the rollouts of several independent samplers (own policy, envs, buffer) in one launch; problem r = blockIdx / E
  const RolloutArgs a = multi ? multi[blockIdx.x / a_single.E] : a_single;
  const int e = multi ? (int)(blockIdx.x % a_single.E) : (int)blockIdx.x, lane = threadIdx.x;
  const NetDesc& nd = a.nd;
  constexpr int SD = KIND == CRUX_ENV_CARTPOLE ? 4 : ((KIND == CRUX_ENV_SYNTH || KIND == CRUX_ENV_SYNTH_DISCRETE) ? IN : 2);
  float w1[IN], w2[64], w3[OUT], b3[OUT];
#pragma unroll
  for (int k = 0; k < IN; ++k) w1[k] = a.p[nd.woff[0] + lane + 64 * k];
#pragma unroll
  for (int k = 0; k < 64; ++k) w2[k] = a.p[nd.woff[1] + lane + 64 * k];
#pragma unroll
  for (int o = 0; o < OUT; ++o) { w3[o] = a.p[nd.woff[2] + o + OUT * lane]; b3[o] = a.p[nd.boff[2] + o]; }
  const float b1 = a.p[nd.boff[0] + lane], b2 = a.p[nd.boff[1] + lane];
  double st[ENV_MAXSD]; float x[IN], nx[ENV_MAXOBS];
#pragma unroll
  for (int i = 0; i < SD; ++i) st[i] = a.state[(size_t)e * SD + i];
  int64_t ep_len = a.ep_len[e], n_resets = a.n_resets[e], steps_taken = a.steps_taken[e]; double sum_r = 0.0; int64_t nee = 0;
#pragma unroll
  for (int k = 0; k < IN; ++k) x[k] = a.svec[(size_t)e * IN + k];
  for (int64_t t = 0; t < a.T; ++t) {
    const int64_t j = (a.base + (int64_t)e * a.T + t) % a.C;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < IN; ++k) a.S[(size_t)j * IN + k] = x[k];
    }
    float z[OUT];
    h64_forward<IN, OUT, ACT>(w1, w2, w3, b3, b1, b2, x, sh, lane, z);
    rollout_tail(a, z, IN, OUT, OUT, KIND, e, t, j, lane == 0, st, ep_len, n_resets, steps_taken, sum_r, nee, nx, lane);
#pragma unroll
    for (int k = 0; k < IN; ++k) x[k] = nx[k];
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < SD; ++i) a.state[(size_t)e * SD + i] = st[i];
    a.ep_len[e] = ep_len; a.n_resets[e] = n_resets; a.steps_taken[e] = steps_taken;
    a.acc[2 * e] = sum_r; a.acc[2 * e + 1] = (double)nee;
#pragma unroll
    for (int k = 0; k < IN; ++k) a.svec[(size_t)e * IN + k] = x[k];
  }
}

__global__ __launch_bounds__(64) void k_rollout(RolloutArgs a) {
  __shared__ float hbuf[2][1024];
  __shared__ float sh_misc[ENV_MAXOBS + 8];
  rollout_generic_wave(a, blockIdx.x, threadIdx.x, hbuf, sh_misc);
}
// one WORKGROUP of 256 threads per environment: thread o evaluates output unit o of a layer (weights W[o + out k] coalesced over the threads, the previous layer
// broadcast from LDS), thread 0 runs the head, the dynamics and the bookkeeping. For policies with layers of 128 units or more.
__global__ __launch_bounds__(256) void k_rollout_wide(RolloutArgs a) {
  __shared__ float hbuf[2][1024];
  __shared__ float sh_misc[ENV_MAXOBS + 8];
  rollout_generic_wave<256>(a, blockIdx.x, threadIdx.x, hbuf, sh_misc);
}
// the two generic kernels for a two-headed Gaussian policy handle (crux_mlp_set_sigma_head): the same body with rollout_head_sigma as its head. Kernels of their own, so that
// k_rollout and k_rollout_wide keep their code and registers
__global__ __launch_bounds__(64) void k_rollout_sigma(RolloutArgs a) {
  __shared__ float hbuf[2][1024];
  __shared__ float sh_misc[ENV_MAXOBS + 8];
  rollout_generic_wave<64, true>(a, blockIdx.x, threadIdx.x, hbuf, sh_misc);
}
__global__ __launch_bounds__(256) void k_rollout_wide_sigma(RolloutArgs a) {
  __shared__ float hbuf[2][1024];
  __shared__ float sh_misc[ENV_MAXOBS + 8];
  rollout_generic_wave<256, true>(a, blockIdx.x, threadIdx.x, hbuf, sh_misc);
}

// ---- register-resident WIDE policy: IN -> H -> H -> OUT with H = 256 or 128 (the off-policy configurations C3 / C4: 8->256->256->4, 3->256->256->1) -------------------------
// One workgroup of 256 threads (one wave per SIMD: up to 512 registers per thread) per environment. Thread o keeps row o of W1 and of W2 -- H weights of the second layer -- in
// registers for the whole launch and evaluates unit o of both hidden layers with the generic kernels' arithmetic (fma over k ascending, + bias, activation: the same bits); the
// output layer's weights sit in LDS. A batch-1 layer streamed from the L2 is a chain of H / (loads in flight) round trips per step (k_rollout_wide: 20 us per step at H = 256);
// from registers it is H fma. steps!(sampler, buffer; Nsteps = dN) of an off-policy solve calls this with T = dN = 4..50 steps per launch.
__device__ __forceinline__ void env_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }      // LDS traffic only: does not wait for the column stores
__device__ __forceinline__ float env_readlane(const float v, const int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
// acc = fma(w[i], h[L0 + i], acc) for i = 0..7, h[l] = lane l of hreg: v_readlane into a scalar register, v_fmac with it as the scalar operand (the product commutes: the bits
// of fmaf(w, h, acc)). Written out because the scheduler, left alone, hoists every v_readlane of a layer and then spills the scalar registers they fill.
template <int L0>
__device__ __forceinline__ void env_rl_fma8(float& acc, const float hreg, const float w0, const float w1, const float w2, const float w3, const float w4, const float w5,
                                            const float w6, const float w7) {
  int t0, t1;
  asm volatile("v_readlane_b32 %[t0], %[h], %[l0]\n\tv_readlane_b32 %[t1], %[h], %[l1]\n\t"
               "v_fmac_f32_e32 %[acc], %[t0], %[w0]\n\tv_readlane_b32 %[t0], %[h], %[l2]\n\t"
               "v_fmac_f32_e32 %[acc], %[t1], %[w1]\n\tv_readlane_b32 %[t1], %[h], %[l3]\n\t"
               "v_fmac_f32_e32 %[acc], %[t0], %[w2]\n\tv_readlane_b32 %[t0], %[h], %[l4]\n\t"
               "v_fmac_f32_e32 %[acc], %[t1], %[w3]\n\tv_readlane_b32 %[t1], %[h], %[l5]\n\t"
               "v_fmac_f32_e32 %[acc], %[t0], %[w4]\n\tv_readlane_b32 %[t0], %[h], %[l6]\n\t"
               "v_fmac_f32_e32 %[acc], %[t1], %[w5]\n\tv_readlane_b32 %[t1], %[h], %[l7]\n\t"
               "v_fmac_f32_e32 %[acc], %[t0], %[w6]\n\tv_fmac_f32_e32 %[acc], %[t1], %[w7]"
               : [acc] "+v"(acc), [t0] "=&s"(t0), [t1] "=&s"(t1)
               : [h] "v"(hreg), [w0] "v"(w0), [w1] "v"(w1), [w2] "v"(w2), [w3] "v"(w3), [w4] "v"(w4), [w5] "v"(w5), [w6] "v"(w6), [w7] "v"(w7),
                 [l0] "n"(L0), [l1] "n"(L0 + 1), [l2] "n"(L0 + 2), [l3] "n"(L0 + 3), [l4] "n"(L0 + 4), [l5] "n"(L0 + 5), [l6] "n"(L0 + 6), [l7] "n"(L0 + 7));
}
template <int H, int K0 = 0>
__device__ __forceinline__ void env_rl_layer(float& acc, const float (&hr)[H / 64], const float (&w)[H]) {
  if constexpr (K0 < H) {
    env_rl_fma8<(K0 & 63)>(acc, hr[K0 >> 6], w[K0], w[K0 + 1], w[K0 + 2], w[K0 + 3], w[K0 + 4], w[K0 + 5], w[K0 + 6], w[K0 + 7]);
    env_rl_layer<H, K0 + 8>(acc, hr, w);
  }
}
template <int H, int K0 = 0>
__device__ __forceinline__ void env_rl_layer_lds(float& acc, const float (&hr)[H / 64], const float* wrow) {      // the weights of the row from LDS, 32 at a time
  if constexpr (K0 < H) {
    float4 wv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) wv[q] = *(const float4*)&wrow[K0 + 4 * q];
    env_rl_fma8<(K0 & 63)>(acc, hr[K0 >> 6], wv[0].x, wv[0].y, wv[0].z, wv[0].w, wv[1].x, wv[1].y, wv[1].z, wv[1].w);
    env_rl_fma8<((K0 + 8) & 63)>(acc, hr[K0 >> 6], wv[2].x, wv[2].y, wv[2].z, wv[2].w, wv[3].x, wv[3].y, wv[3].z, wv[3].w);
    env_rl_fma8<((K0 + 16) & 63)>(acc, hr[K0 >> 6], wv[4].x, wv[4].y, wv[4].z, wv[4].w, wv[5].x, wv[5].y, wv[5].z, wv[5].w);
    env_rl_fma8<((K0 + 24) & 63)>(acc, hr[K0 >> 6], wv[6].x, wv[6].y, wv[6].z, wv[6].w, wv[7].x, wv[7].y, wv[7].z, wv[7].w);
    env_rl_layer_lds<H, K0 + 32>(acc, hr, wrow);
  }
}
template <int H>
__global__ __launch_bounds__(256) void k_rollout_res(RolloutArgs a) {
  __shared__ __attribute__((aligned(16))) float hb[2][H];      // the hidden activations of the two layers
  __shared__ __attribute__((aligned(16))) float w3s[4 * (H + 4)];      // row o of W3 contiguous (+4: the nout <= 4 rows start in different banks)
  __shared__ float xin[ENV_MAXOBS], smu[8], ssg[8];
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
#ifdef CRUX_RES_TIMING
  const long long t_entry = wall_clock64();
#endif
  const NetDesc& nd = a.nd; const int od = a.od, nout = nd.dims[3];
  const bool on = tid < H;
  float w1[8], w2[H];      // (obs_dim <= 8 for the shapes dispatched here)
#pragma unroll
  for (int k = 0; k < 8; ++k) w1[k] = (on && k < od) ? a.p[nd.woff[0] + tid + H * k] : 0.f;
  // (element by element: 256-byte loads per wave, ~64 KB in flight per compute unit -- 10 us for the 256 KB of H = 256. Wider pieces dealt to their owners through LDS need the
  //  registers twice or > 64 KB of staging to keep enough bytes in flight; measured slower within the static 64 KB)
#pragma unroll
  for (int k = 0; k < H; ++k) w2[k] = on ? a.p[nd.woff[1] + tid + H * k] : 0.f;
  const float b1 = on ? a.p[nd.boff[0] + tid] : 0.f, b2 = on ? a.p[nd.boff[1] + tid] : 0.f;
  for (int q = tid; q < nout * H; q += 256) w3s[(q % nout) * (H + 4) + q / nout] = a.p[nd.woff[2] + q];      // W3[o + nout k] in the flat vector -> row o
  const int row3 = lane < nout ? lane : 0;
  const float b3 = a.p[nd.boff[2] + row3];
  const int act1 = nd.acts[0], act2 = nd.acts[1], act3 = nd.acts[2];
  // wave 0 carries the sampler state, identically in every lane (the head, the dynamics and the bookkeeping are evaluated redundantly; lane 0 writes)
  double st[ENV_MAXSD]; int64_t ep_len = 0, n_resets = 0, steps_taken = 0; double sum_r = 0.0; int64_t nee = 0;
  if (tid < 64) {
#pragma unroll
    for (int i = 0; i < ENV_MAXSD; ++i) if (i < a.sd) st[i] = a.state[(size_t)e * a.sd + i];
    ep_len = a.ep_len[e]; n_resets = a.n_resets[e]; steps_taken = a.steps_taken[e]; }
  if (tid < od) { xin[tid] = a.svec[(size_t)e * od + tid]; smu[tid] = a.mu[tid]; ssg[tid] = a.sigma[tid]; }
  __syncthreads();
#ifdef CRUX_RES_TIMING
  long long tk[6] = {0, 0, 0, 0, 0, 0}, t0 = wall_clock64(), t1;
#define RT(i) { t1 = wall_clock64(); tk[i] += t1 - t0; t0 = t1; }
#else
#define RT(i)
#endif
  int64_t j = (a.base + (int64_t)e * a.T) % a.C;      // the ring row of step t: (base + e T + t) % C, advanced instead of divided
  for (int64_t t = 0; t < a.T; ++t, j = j + 1 == a.C ? 0 : j + 1) {
    if (tid < od) a.S[(size_t)j * od + tid] = xin[tid];      // current observation -> S column (sampler.jl:100)
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) if (k < od) acc = fmaf(w1[k], xin[k], acc);
    if (on) hb[0][tid] = crux_act(act1, acc + b1);
    env_lds_barrier();
    RT(0)
    // layer 2: the H activations sit H / 64 per lane; v_readlane broadcasts h[k] as the scalar operand of the fma (an LDS broadcast read per k is a round trip per k)
    float hr[H / 64];
#pragma unroll
    for (int c = 0; c < H / 64; ++c) hr[c] = hb[0][lane + 64 * c];
    acc = 0.f;
    env_rl_layer<H>(acc, hr, w2);
    if (on) hb[1][tid] = crux_act(act2, acc + b2);
    env_lds_barrier();
    RT(1)
    if (tid < 64) {      // wave 0: the output layer (lane o = unit o; the other lanes repeat unit 0), then everything of step! after the forward pass
#pragma unroll
      for (int c = 0; c < H / 64; ++c) hr[c] = hb[1][lane + 64 * c];
      float z = 0.f;
      env_rl_layer_lds<H>(z, hr, &w3s[row3 * (H + 4)]);
      z = crux_act(act3, z + b3);
      RT(2)
      float zz[4], nx[ENV_MAXOBS];
      // (the host dispatches here only for these two environment shapes)
      if (a.kind == CRUX_ENV_PENDULUM) { zz[0] = env_readlane(z, 0);
        rollout_tail(a, zz, 3, 1, 1, CRUX_ENV_PENDULUM, e, t, j, tid == 0, st, ep_len, n_resets, steps_taken, sum_r, nee, nx, lane, smu, ssg);
        if (tid == 0) { xin[0] = nx[0]; xin[1] = nx[1]; xin[2] = nx[2]; } }
      else { zz[0] = env_readlane(z, 0); zz[1] = env_readlane(z, 1); zz[2] = env_readlane(z, 2); zz[3] = env_readlane(z, 3);
        rollout_tail(a, zz, 8, 4, 4, CRUX_ENV_SYNTH_DISCRETE, e, t, j, tid == 0, st, ep_len, n_resets, steps_taken, sum_r, nee, nx, lane, smu, ssg);
        if (tid == 0) {
#pragma unroll
          for (int q = 0; q < 8; ++q) xin[q] = nx[q]; } }
      RT(3)
    }
    env_lds_barrier();
    RT(4)
  }
#ifdef CRUX_RES_TIMING
  if (tid == 0 && e == 0) printf("[res-timing] prologue %lld\n", t0 - t_entry - tk[0] - tk[1] - tk[2] - tk[3] - tk[4]);
  if (tid == 0 && e == 0) printf("[res-timing] T=%lld ticks: l1 %lld l2 %lld l3 %lld tail %lld bar %lld\n", (long long)a.T, tk[0], tk[1], tk[2], tk[3], tk[4]);
#endif
#undef RT
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < ENV_MAXSD; ++i) if (i < a.sd) a.state[(size_t)e * a.sd + i] = st[i];
    a.ep_len[e] = ep_len; a.n_resets[e] = n_resets; a.steps_taken[e] = steps_taken;
    a.acc[2 * e] = sum_r; a.acc[2 * e + 1] = (double)nee; }
  if (tid < od) a.svec[(size_t)e * od + tid] = xin[tid];
  // the T rows just written get the maximal priority (experience_buffer.jl:254), in this launch (one environment: the rows are this workgroup's)
#ifdef CRUX_RES_TIMING
  const long long tp0 = wall_clock64();
#endif
  if (a.pt_pr) { if (a.pt_touch && a.T <= PUSH_SMALL_MAX && a.T <= a.C) push_touch_small(a.pt_ids, (int)a.T, a.base, a.C, a.pt_pr, a.pt_pminmax, a.pt_alpha, a.pt_N, a.pt_nlev, a.pt_run, a.pt_total);
    else push_touch_block(a.pt_ids, a.T, a.base, a.C, a.pt_pr, a.pt_pminmax, a.pt_alpha, a.pt_N, a.pt_nlev, a.pt_run, a.pt_total, a.pt_touch); }
#ifdef CRUX_RES_TIMING
  if (tid == 0 && e == 0) printf("[res-timing] push %lld ticks (touch %d)\n", wall_clock64() - tp0, a.pt_touch);
#endif
}

// ---- caller-stepped environments: step! with an arbitrary mdp on the host (sampler.jl:71-137) ----------------------------------------------------------------
// The reference's step! calls @gen(:sp,:r)(mdp, s, a) on whatever mdp the user handed to solve (sampler.jl:89-97). For environments that only exist on the host the
// device part of a step is the policy: exploration(pi_explore, svec; pi_on, i) / action(pi, svec) (sampler.jl:73) for the E current observations at once --
// a.svec = observations [od x E], a.steps_taken = draws each sampler has made so far, a.cfg.i0 = the interaction counter of sampler 0; outputs a.A (one-hot bytes or
// Float32 [ad x E]) and a.LP [E]. The forward pass and the head are the rollout kernels' own (h64_forward / rollout_generic_forward, rollout_head): a caller that steps the
// restated CartPole on the host gets the transitions crux_rollout produces, bit for bit (tests/test_gpu_host_env.py).
__device__ __forceinline__ void explore_store(const RolloutArgs& a, const int e, const int ad, const float* aout, const float logprob) {
  if (a.act_kind == CRUX_ACTION_DISCRETE) { uint8_t* A = (uint8_t*)a.A + (size_t)e * ad; for (int q = 0; q < ad; ++q) A[q] = aout[q] != 0.f; }
  else { float* A = (float*)a.A + (size_t)e * ad; for (int q = 0; q < ad; ++q) A[q] = aout[q]; }
  a.LP[e] = logprob;
}
template <int IN, int OUT, int ACT>
__global__ __launch_bounds__(64) void k_explore_h64(RolloutArgs a) {
  __shared__ __attribute__((aligned(16))) float sh[64];
  const int e = blockIdx.x, lane = threadIdx.x;
  const NetDesc& nd = a.nd;
  float w1[IN], w2[64], w3[OUT], b3[OUT], x[IN], z[OUT];
#pragma unroll
  for (int k = 0; k < IN; ++k) w1[k] = a.p[nd.woff[0] + lane + 64 * k];
#pragma unroll
  for (int k = 0; k < 64; ++k) w2[k] = a.p[nd.woff[1] + lane + 64 * k];
#pragma unroll
  for (int o = 0; o < OUT; ++o) { w3[o] = a.p[nd.woff[2] + o + OUT * lane]; b3[o] = a.p[nd.boff[2] + o]; }
  const float b1 = a.p[nd.boff[0] + lane], b2 = a.p[nd.boff[1] + lane];
#pragma unroll
  for (int k = 0; k < IN; ++k) x[k] = a.svec[(size_t)e * IN + k];
  h64_forward<IN, OUT, ACT>(w1, w2, w3, b3, b1, b2, x, sh, lane, z);
  float aout[ENV_MAXOBS]; int ai; float logprob;
  rollout_head(a, z, OUT, OUT, e, a.cfg.i0 + (uint64_t)e, (uint64_t)a.steps_taken[e], aout, ai, logprob);
  if (lane == 0) explore_store(a, e, OUT, aout, logprob);
}
template <int NT>
__global__ __launch_bounds__(NT) void k_explore_generic(RolloutArgs a) {
  __shared__ float hbuf[2][1024];
  const int e = blockIdx.x, lane = threadIdx.x, od = a.od, nout = a.nd.dims[a.nd.L];
  if (lane < od) hbuf[0][lane] = a.svec[(size_t)e * od + lane];
  if (NT == 64) { RO_WAVE_SYNC(); } else { __syncthreads(); }
  const int cur = rollout_generic_forward<NT>(a, lane, hbuf);
  if (lane == 0) { float aout[ENV_MAXOBS]; int ai; float logprob;
    if (a.sigma_head) rollout_head_sigma(a, hbuf[cur], a.ad, e, (uint64_t)a.steps_taken[e], aout, ai, logprob); else
    rollout_head(a, hbuf[cur], a.ad, nout, e, a.cfg.i0 + (uint64_t)e, (uint64_t)a.steps_taken[e], aout, ai, logprob);
    explore_store(a, e, a.ad, aout, logprob); }
}

__global__ void k_env_init(int kind, int E, int od, int sd, uint64_t seed, const float* mu, const float* sigma, double* state, int64_t* ep_len,
                           int64_t* n_resets, float* svec, int fresh) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t nr = fresh ? 0 : n_resets[e];
  if (env_is_synth(kind)) {                                  // straight to memory: no per-thread arrays (observation i == state i)
    for (int i = 0; i < sd; ++i) { const crux_u32x4 x = crux_philox(seed, 16 * (uint64_t)nr + (uint64_t)(i >> 1), (uint32_t)e, CRUX_RNG_RESET);
      const double ui = (i & 1) ? crux_u32x2_to_f64(x.v[2], x.v[3]) : crux_u32x2_to_f64(x.v[0], x.v[1]); const double xi = __dadd_rn(-0.05, __dmul_rn(0.1, ui));
      state[(size_t)e * sd + i] = xi; svec[(size_t)e * od + i] = __fdiv_rn(__fsub_rn((float)xi, mu[i]), sigma[i]); }
    n_resets[e] = nr + 1; ep_len[e] = 0; return;
  }
  double st[4]; float o[4];
  st[0] = st[1] = st[2] = st[3] = 0.0; o[0] = o[1] = o[2] = o[3] = 0.f;
  env_draw_initial(kind, seed, (uint64_t)nr, (uint32_t)e, st);
#pragma unroll
  for (int i = 0; i < 4; ++i) if (i < sd) state[(size_t)e * sd + i] = st[i];      // static indices: keep the arrays in registers
  n_resets[e] = nr + 1; ep_len[e] = 0;
  env_obs(kind, st, o);
#pragma unroll
  for (int q = 0; q < 4; ++q) if (q < od) svec[(size_t)e * od + q] = __fdiv_rn(__fsub_rn(o[q], mu[q]), sigma[q]);
}

__global__ void k_env_step(int kind, int64_t n, const double* state, const void* action, const double* uniforms, double* next_state, float* obs, float* r, uint8_t* done) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (kind == CRUX_ENV_GRIDWORLD) {
    const uint8_t* a = (const uint8_t*)action + 4 * j; int act = 0; for (int q = 0; q < 4; ++q) if (a[q]) act = q;
    double s[2] = {state[2 * j], state[2 * j + 1]}, sn[2]; float rr; uint8_t dd;
    gridworld_step(s, act, uniforms ? uniforms[j] : 0.0, sn, &rr, &dd);
    next_state[2 * j] = sn[0]; next_state[2 * j + 1] = sn[1]; obs[2 * j] = (float)sn[0]; obs[2 * j + 1] = (float)sn[1]; r[j] = rr; done[j] = dd; return;
  }
  if (kind == CRUX_ENV_CARTPOLE) {
    const uint8_t* a = (const uint8_t*)action + 2 * j; double s[4], sn[4]; for (int i = 0; i < 4; ++i) s[i] = state[4 * j + i];
    float rr; uint8_t dd; cartpole_step(s, a[1] ? 1 : 0, sn, &rr, &dd);
    for (int i = 0; i < 4; ++i) { next_state[4 * j + i] = sn[i]; obs[4 * j + i] = (float)sn[i]; } r[j] = rr; done[j] = dd;
  } else {
    double s[2] = {state[2 * j], state[2 * j + 1]}, sn[2]; float rr; uint8_t dd; float o[3];
    pendulum_step(s, ((const float*)action)[j], sn, &rr, &dd); env_obs(kind, sn, o);
    next_state[2 * j] = sn[0]; next_state[2 * j + 1] = sn[1]; obs[3 * j] = o[0]; obs[3 * j + 1] = o[1]; obs[3 * j + 2] = o[2]; r[j] = rr; done[j] = dd;
  }
}

static void env_dims(int kind, int so, int sa, int* obs, int* act, int* sd) {
  switch (kind) {
    case CRUX_ENV_CARTPOLE: *obs = 4; *act = 2; *sd = 4; break;
    case CRUX_ENV_PENDULUM: *obs = 3; *act = 1; *sd = 2; break;
    case CRUX_ENV_GRIDWORLD: *obs = 2; *act = 4; *sd = 2; break;
    case CRUX_ENV_SYNTH: case CRUX_ENV_SYNTH_DISCRETE: *obs = so; *act = sa; *sd = so; break;
    default: *obs = so; *act = sa; *sd = 1; break;
  }
}

// k_rollout_h64 for an is_h64 policy on environment `kind` (false: no row of the shape table). d_multi: the device array of per-problem arguments of a batched launch, or NULL
static bool launch_rollout_h64(const NetDesc& pn, int kind, dim3 grid, hipStream_t stream, const RolloutArgs& a, const RolloutArgs* d_multi) {
#define RO_CASE(I, O, A_, K) if (pn.dims[0] == I && pn.dims[3] == O && pn.acts[0] == A_ && kind == K) { hipLaunchKernelGGL((k_rollout_h64<I, O, A_, K>), grid, dim3(64), 0, stream, a, d_multi); return true; }
  H64_SHAPES(RO_CASE)
#undef RO_CASE
  return false;
}

extern "C" {

int32_t crux_env_create(crux_ctx* ctx, int32_t kind, int32_t n_envs, int32_t max_steps, float gamma, const float* obs_mu, const float* obs_sigma,
                        uint64_t seed, int32_t synth_obs_dim, int32_t synth_act_dim, crux_env** out) {
  if (!ctx || !out) return CRUX_EINVAL;
  if (kind < CRUX_ENV_CARTPOLE || kind > CRUX_ENV_SYNTH_DISCRETE) return crux_fail(ctx, CRUX_EUNSUP, "env kind %d has no device dynamics", kind);
  if ((kind == CRUX_ENV_SYNTH || kind == CRUX_ENV_SYNTH_DISCRETE) && (synth_obs_dim < 1 || synth_obs_dim > ENV_MAXOBS || synth_act_dim < 1 || synth_act_dim > ENV_MAXOBS))
    return crux_fail(ctx, CRUX_EINVAL, "synthetic env: obs/act dims (%d, %d) must be in 1..%d", synth_obs_dim, synth_act_dim, ENV_MAXOBS);
  if (n_envs < 1 || max_steps < 1) return crux_fail(ctx, CRUX_EINVAL, "env_create: n_envs=%d max_steps=%d", n_envs, max_steps);
  crux_env* e = new crux_env(); e->ctx = ctx; e->kind = kind; e->n_envs = n_envs; e->max_steps = max_steps; e->gamma = gamma; e->seed = seed;
  env_dims(kind, synth_obs_dim, synth_act_dim, &e->obs_dim, &e->act_dim, &e->state_dim);
  const int od = e->obs_dim;
  if (hipMalloc(&e->mu, 4 * od) != hipSuccess || hipMalloc(&e->sigma, 4 * od) != hipSuccess || hipMalloc(&e->state, 8 * (size_t)n_envs * e->state_dim) != hipSuccess ||
      hipMalloc(&e->ep_len, 8 * (size_t)n_envs) != hipSuccess || hipMalloc(&e->n_resets, 8 * (size_t)n_envs) != hipSuccess ||
      hipMalloc(&e->steps_taken, 8 * (size_t)n_envs) != hipSuccess || hipMalloc(&e->svec, 4 * (size_t)n_envs * od) != hipSuccess ||
      hipMalloc(&e->acc, 16 * (size_t)n_envs) != hipSuccess) { crux_env_destroy(e); return crux_fail(ctx, CRUX_ENOMEM, "env_create: hipMalloc"); }
  std::vector<float> mu(od, 0.f), sg(od, 1.f);
  if (obs_mu) for (int i = 0; i < od; ++i) mu[i] = obs_mu[i];
  if (obs_sigma) for (int i = 0; i < od; ++i) sg[i] = obs_sigma[i];
  HIPCHK(ctx, hipMemcpyAsync(e->mu, mu.data(), 4 * od, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(e->sigma, sg.data(), 4 * od, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(e->steps_taken, 0, 8 * (size_t)n_envs, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(e->acc, 0, 16 * (size_t)n_envs, ctx->stream));
  hipLaunchKernelGGL(k_env_init, dim3((n_envs + 63) / 64), dim3(64), 0, ctx->stream, kind, n_envs, od, e->state_dim, seed, e->mu, e->sigma, e->state, e->ep_len, e->n_resets, e->svec, 1);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *out = e; return crux_launch_check(ctx, "k_env_init");
}

int32_t crux_env_destroy(crux_env* e) {
  if (!e) return CRUX_OK;
  crux_sync_before_free(e->ctx);
  (void)hipFree(e->mu); (void)hipFree(e->sigma); (void)hipFree(e->state); (void)hipFree(e->ep_len); (void)hipFree(e->n_resets);
  (void)hipFree(e->steps_taken); (void)hipFree(e->svec); (void)hipFree(e->acc);
  delete e; return CRUX_OK;
}
int32_t crux_env_obs_dim(const crux_env* e) { return e ? e->obs_dim : -1; }
int32_t crux_env_act_dim(const crux_env* e) { return e ? e->act_dim : -1; }
int32_t crux_env_state_dim(const crux_env* e) { return e ? e->state_dim : -1; }

int32_t crux_env_reset(crux_env* e) {
  if (!e) return CRUX_EINVAL;
  hipLaunchKernelGGL(k_env_init, dim3((e->n_envs + 63) / 64), dim3(64), 0, e->ctx->stream, e->kind, e->n_envs, e->obs_dim, e->state_dim, e->seed, e->mu, e->sigma,
                     e->state, e->ep_len, e->n_resets, e->svec, 0);
  return crux_launch_check(e->ctx, "k_env_init");
}

int32_t crux_env_get_state(crux_env* e, double* state, int64_t* ep_len, int64_t* n_resets) {
  if (!e) return CRUX_EINVAL;
  crux_ctx* c = e->ctx;
  if (state) HIPCHK(c, hipMemcpyAsync(state, e->state, 8 * (size_t)e->n_envs * e->state_dim, hipMemcpyDeviceToHost, c->stream));
  if (ep_len) HIPCHK(c, hipMemcpyAsync(ep_len, e->ep_len, 8 * (size_t)e->n_envs, hipMemcpyDeviceToHost, c->stream));
  if (n_resets) HIPCHK(c, hipMemcpyAsync(n_resets, e->n_resets, 8 * (size_t)e->n_envs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CRUX_OK;
}

int32_t crux_rollout(crux_env* e, crux_mlp* policy, const crux_rollout_cfg* cfg, crux_buffer* buf, int64_t T, double* sum_r, int64_t* n_episode_end) { CRUX_PLAIN_ONLY("crux_rollout", policy);
  if (!e || !policy || !cfg || !buf || T < 1) return CRUX_EINVAL;
  crux_ctx* c = e->ctx;
  const int64_t N = (int64_t)e->n_envs * T;
  if (buf->obs_dim != e->obs_dim || buf->act_dim != e->act_dim) return crux_fail(c, CRUX_EINVAL, "steps!: buffer columns (%d,%d) do not match the env (%d,%d)", buf->obs_dim, buf->act_dim, e->obs_dim, e->act_dim);
  if (N > buf->capacity) return crux_fail(c, CRUX_EINVAL, "steps!: %lld transitions exceed buffer capacity %lld", (long long)N, (long long)buf->capacity);
  if (policy->nd.dims[0] != e->obs_dim) return crux_fail(c, CRUX_EINVAL, "steps!: policy input %d != obs dim %d", policy->nd.dims[0], e->obs_dim);
  if (policy->nd.maxdim > 1024) return crux_fail(c, CRUX_EUNSUP, "steps!: layer width %d > 1024", policy->nd.maxdim);
  const int nout = policy->nd.dims[policy->nd.L];
  if ((cfg->head == CRUX_HEAD_CATEGORICAL || cfg->head == CRUX_HEAD_GREEDY_Q) && (nout != e->act_dim || buf->act_kind != CRUX_ACTION_DISCRETE))
    return crux_fail(c, CRUX_EINVAL, "steps!: discrete head needs %d logits and a one-hot action column", e->act_dim);
  const bool two = policy->sigma_head;      // two-headed Gaussian handle: 2 act_dim outputs [mu; logSigma], no extras; the generic kernels only
  if (two && ((cfg->head != CRUX_HEAD_GAUSSIAN && cfg->head != CRUX_HEAD_DETERMINISTIC) || nout != 2 * e->act_dim || policy->nd.n_extra != 0 || buf->act_kind != CRUX_ACTION_CONTINUOUS))
    return crux_fail(c, CRUX_EINVAL, "steps!: a two-headed Gaussian policy needs a continuous head, 2 x %d outputs, no extras and a Float32 action column", e->act_dim);
  if (!two && (cfg->head == CRUX_HEAD_GAUSSIAN || cfg->head == CRUX_HEAD_DETERMINISTIC) && (nout != e->act_dim || buf->act_kind != CRUX_ACTION_CONTINUOUS))
    return crux_fail(c, CRUX_EINVAL, "steps!: continuous head needs %d outputs and a Float32 action column", e->act_dim);
  if (!two && cfg->head == CRUX_HEAD_GAUSSIAN && policy->nd.n_extra != e->act_dim) return crux_fail(c, CRUX_EINVAL, "steps!: GaussianPolicy needs %d logSigma extras", e->act_dim);
  RolloutArgs a; fill_rollout_args(a, e, policy, cfg, buf, T);
  crux_prof_begin(c, CRUX_PROF_ROLLOUT);
  const NetDesc& pn = policy->nd;
  bool push_done = false; int pt_touch = 0;
  if (two) {      // never a register-resident form (a 3-64-64-2 Pendulum actor has an instantiated shape by its dims)
    if (policy->nd.maxdim >= 128) hipLaunchKernelGGL(k_rollout_wide_sigma, dim3(e->n_envs), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(k_rollout_sigma, dim3(e->n_envs), dim3(64), 0, c->stream, a); } else
  if (is_h64(pn) && !crux_sw().force_generic && launch_rollout_h64(pn, e->kind, dim3(e->n_envs), c->stream, a, nullptr)) {} else
  // wide two-hidden-layer policies (C3 / C4): the register-resident kernel when the launch is long enough to pay for loading W2 into registers (a step costs 8 round trips
  // streamed; the load costs 8 once) -- always, from two steps on
  if (pn.L == 3 && pn.dims[1] == pn.dims[2] && (pn.dims[1] == 256 || pn.dims[1] == 128) && T >= 2 && !crux_sw().force_generic &&
      ((e->kind == CRUX_ENV_PENDULUM && e->obs_dim == 3 && e->act_dim == 1 && nout == 1) || (e->kind == CRUX_ENV_SYNTH_DISCRETE && e->obs_dim == 8 && e->act_dim == 4 && nout == 4))) {
    if (e->n_envs == 1 && crux_per_push_plan(buf, N, &pt_touch)) { push_done = true;
      a.pt_ids = buf->d_indices; a.pt_pr = buf->priorities; a.pt_pminmax = buf->pminmax; a.pt_run = buf->cumsum; a.pt_total = buf->topo_total; a.pt_alpha = buf->alpha;
      a.pt_nlev = (int32_t)buf->topo_levels; a.pt_touch = pt_touch; a.pt_N = (int64_t)buf->topo_n; }
    if (pn.dims[1] == 256) hipLaunchKernelGGL(k_rollout_res<256>, dim3(e->n_envs), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(k_rollout_res<128>, dim3(e->n_envs), dim3(256), 0, c->stream, a); }
  else if (policy->nd.maxdim >= 128) hipLaunchKernelGGL(k_rollout_wide, dim3(e->n_envs), dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL(k_rollout, dim3(e->n_envs), dim3(64), 0, c->stream, a);
  crux_prof_end(c, CRUX_PROF_ROLLOUT);
  int32_t rc = crux_launch_check(c, "k_rollout"); if (rc) return rc;
  if (push_done) crux_per_push_done(buf, pt_touch);
  else if (buf->prioritized) {      // push!: the new rows get max_priority (experience_buffer.jl:254); their ring rows are formed on the device, nothing to wait for
    if (crux_per_push_fused(buf, N, buf->d_indices)) { rc = crux_launch_check(c, "k_push_touch"); if (rc) return rc; }      // a few rows: the whole bookkeeping as one launch
    else {
      rc = crux_buffer_ring_ids_device(buf, N, buf->d_indices); if (rc) return rc;
      rc = crux_buffer_per_on_push(buf, buf->d_indices, N); if (rc) return rc; }
  }
  crux_buffer_ring_advance(buf, N);
  if (sum_r || n_episode_end) {
    std::vector<double> acc(2 * (size_t)e->n_envs);
    HIPCHK(c, hipMemcpyAsync(acc.data(), e->acc, 16 * (size_t)e->n_envs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rollout_acc_sum(acc.data(), e->n_envs, sum_r, n_episode_end);
  }
  return CRUX_OK;
}

// exploration(pi_explore, svec; pi_on, i) / action(pi, svec) of step! (sampler.jl:73) for n_envs caller-stepped samplers at once: see k_explore_* above.
int32_t crux_policy_explore(crux_mlp* policy, const crux_rollout_cfg* cfg, int32_t n_envs, const float* obs, uint64_t seed, const int64_t* steps_taken,
                            void* actions_out, float* logprob_out) { CRUX_PLAIN_ONLY("crux_policy_explore", policy);
  if (!policy || !cfg || !obs || !actions_out || n_envs < 1) return CRUX_EINVAL;
  crux_ctx* c = policy->ctx; const NetDesc& pn = policy->nd;
  if (pn.L < 1) return crux_fail(c, CRUX_EINVAL, "policy_explore: the policy has no layers");
  const bool two = policy->sigma_head; const int od = pn.dims[0], nout = two ? pn.dims[pn.L] / 2 : pn.dims[pn.L];      // (two-headed: nout = act_dim, the rows of an action)
  if (od > ENV_MAXOBS || nout > ENV_MAXOBS) return crux_fail(c, CRUX_EUNSUP, "policy_explore: observation / action widths (%d, %d) above %d", od, nout, ENV_MAXOBS);
  if (pn.maxdim > 1024) return crux_fail(c, CRUX_EUNSUP, "policy_explore: layer width %d > 1024", pn.maxdim);
  if (cfg->head < CRUX_HEAD_CATEGORICAL || cfg->head > CRUX_HEAD_DETERMINISTIC) return crux_fail(c, CRUX_EINVAL, "policy_explore: head %d", cfg->head);
  if (two && ((cfg->head != CRUX_HEAD_GAUSSIAN && cfg->head != CRUX_HEAD_DETERMINISTIC) || pn.n_extra != 0)) return crux_fail(c, CRUX_EINVAL, "policy_explore: a two-headed Gaussian policy needs a continuous head and no extras");
  if (!two && cfg->head == CRUX_HEAD_GAUSSIAN && pn.n_extra != nout) return crux_fail(c, CRUX_EINVAL, "policy_explore: GaussianPolicy needs %d logSigma extras", nout);
  const bool disc = cfg->head == CRUX_HEAD_CATEGORICAL || cfg->head == CRUX_HEAD_GREEDY_Q;
  const size_t E = (size_t)n_envs, b_obs = (4 * E * od + 255) / 256 * 256, b_st = (8 * E + 255) / 256 * 256, b_act = (E * nout * (disc ? 1 : 4) + 255) / 256 * 256, b_lp = (4 * E + 255) / 256 * 256;
  // ONE launch per call: observations, step counters, actions and log-probabilities live in a pinned, device-mapped block of the context -- the kernel
  // reads the E observations straight from host memory and writes the E actions back into it (a few hundred bytes to a few KB over the link, inside the launch) instead of
  // two staged uploads before and two read-backs after the kernel: five dependent stream operations (~60-80 us per call from pageable memory) become one.
  const bool zc = crux_sw().host_zerocopy;      // "0": the round-5 form (device scratch, two staged uploads, two read-backs) -- kept for the A/B of bench_hostenv.py and a bit-identity test
  char* hs = zc ? (char*)crux_pinned_mapped(c, b_obs + b_st + b_act + b_lp) : nullptr; if (zc && !hs) return crux_fail(c, CRUX_ENOMEM, "policy_explore: pinned staging");
  char* sc = zc ? (char*)c->pinned_mapped_dev : (char*)crux_scratch(c, b_obs + b_st + b_act + b_lp); if (!sc) return crux_fail(c, CRUX_ENOMEM, "policy_explore: scratch");
  RolloutArgs a = RolloutArgs{};
  a.nd = pn; a.p = policy->p; a.E = n_envs; a.od = od; a.ad = nout; a.act_kind = disc ? CRUX_ACTION_DISCRETE : CRUX_ACTION_CONTINUOUS; a.seed = seed;
  a.svec = (float*)sc; a.steps_taken = (int64_t*)(sc + b_obs); a.A = sc + b_obs + b_st; a.LP = (float*)(sc + b_obs + b_st + b_act); a.cfg = *cfg; a.squash = policy->squash; a.sigma_head = two ? 1 : 0;
  if (zc) { memcpy(hs, obs, 4 * E * od);
    if (steps_taken) memcpy(hs + b_obs, steps_taken, 8 * E); else memset(hs + b_obs, 0, 8 * E); }
  else { HIPCHK(c, hipMemcpyAsync(a.svec, obs, 4 * E * od, hipMemcpyHostToDevice, c->stream));
    if (steps_taken) HIPCHK(c, hipMemcpyAsync(a.steps_taken, steps_taken, 8 * E, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(a.steps_taken, 0, 8 * E, c->stream)); }
  // the arithmetic of the rollout kernel that serves this policy shape (crux_rollout: the register-resident form for the instantiated IN-64-64-OUT shapes, else the generic one)
  const bool h64 = is_h64(pn) && !two && !crux_sw().force_generic;      // (a 3-64-64-2 two-headed Pendulum actor has an instantiated shape: never the register-resident form)
#define EX_CASE(I, O, A_, K) if (h64 && od == I && nout == O && pn.acts[0] == A_) hipLaunchKernelGGL((k_explore_h64<I, O, A_>), dim3(n_envs), dim3(64), 0, c->stream, a); else
  H64_SHAPES(EX_CASE)
#undef EX_CASE
  if (pn.maxdim >= 128) hipLaunchKernelGGL(k_explore_generic<256>, dim3(n_envs), dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL(k_explore_generic<64>, dim3(n_envs), dim3(64), 0, c->stream, a);
  int32_t rc = crux_launch_check(c, "k_explore"); if (rc) return rc;
  if (!zc) { HIPCHK(c, hipMemcpyAsync(actions_out, a.A, E * nout * (disc ? 1 : 4), hipMemcpyDeviceToHost, c->stream));
    if (logprob_out) HIPCHK(c, hipMemcpyAsync(logprob_out, a.LP, 4 * E, hipMemcpyDeviceToHost, c->stream)); }
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the one synchronisation of the call: the actions are what the caller steps its environment with
  if (zc) { memcpy(actions_out, hs + b_obs + b_st, E * nout * (disc ? 1 : 4));
    if (logprob_out) memcpy(logprob_out, hs + b_obs + b_st + b_act, 4 * E); }
  return CRUX_OK;
}

// the tail of steps! for a block the CALLER stepped (sampler.jl:139-155): push!(buffer, data) of the n transitions (ring write, experience_buffer.jl:232-259) and, on the ring rows
// just written, what terminate_episode! ran on the reference's `data` before the push (sampler.jl:53-66): fill_gae! / fill_returns!, the importance-weight products, the cost
// advantage / return -- for whichever of those columns the buffer has. cols[CRUX_COL_EPISODE_END] carries the caller's episode cuts (done, max_steps, the reset at the end).
int32_t crux_steps_push(crux_buffer* buf, int64_t n, const void* const* cols, int64_t rows_per_env, int32_t close_last, crux_mlp* critic, float lambda, float gamma,
                        crux_mlp* cost_critic, crux_mlp* nominal, int32_t nominal_head, int64_t* first_row_out) { CRUX_PLAIN_ONLY("crux_steps_push", critic, cost_critic, nominal);
  if (!buf || !cols || n < 0) return CRUX_EINVAL;
  crux_ctx* c = buf->ctx;
  if (nominal && nominal->sigma_head) return crux_fail(c, CRUX_EUNSUP, "steps_push: a two-headed Gaussian actor (logSigma network) as the nominal policy of :importance_weight is not implemented");
  if (n > buf->capacity && (has_col(buf, CRUX_COL_ADVANTAGE) || has_col(buf, CRUX_COL_RETURN) || has_col(buf, CRUX_COL_COST_ADVANTAGE) || has_col(buf, CRUX_COL_COST_RETURN) ||
                            has_col(buf, CRUX_COL_FWD_IMPORTANCE_WEIGHT) || has_col(buf, CRUX_COL_CUM_IMPORTANCE_WEIGHT) || has_col(buf, CRUX_COL_REV_IMPORTANCE_WEIGHT) || (nominal && has_col(buf, CRUX_COL_IMPORTANCE_WEIGHT))))
    return crux_fail(c, CRUX_EINVAL, "steps!: a block of %lld transitions does not fit the buffer (capacity %lld) whose advantage / return / importance-weight columns it must fill", (long long)n, (long long)buf->capacity);
  if (!cols[CRUX_COL_EPISODE_END]) return crux_fail(c, CRUX_EINVAL, "steps_push: the block needs its :episode_end column (the caller's Sampler cuts the episodes: sampler.jl:130-136,148)");
  // every argument is checked BEFORE the ring moves: a failed call must not leave pushed rows whose advantage / return columns hold stale data
  if (n > 0 && n <= buf->capacity) {
    if (has_col(buf, CRUX_COL_ADVANTAGE) && !critic) return crux_fail(c, CRUX_EINVAL, "steps_push: the buffer has an :advantage column but no critic was given (fill_gae!, sampler.jl:56)");
    if (has_col(buf, CRUX_COL_COST_ADVANTAGE) && !cost_critic) return crux_fail(c, CRUX_EINVAL, "steps_push: the buffer has a :cost_advantage column but no cost critic (Sampler.Vc, sampler.jl:65)"); }
  const int64_t first = buf->next_ind;
  if (first_row_out) *first_row_out = first;
  int32_t rc = crux_buffer_push_host(buf, n, cols, nullptr); if (rc) return rc;
  if (n == 0 || n > buf->capacity) return CRUX_OK;
  if (has_col(buf, CRUX_COL_ADVANTAGE)) {
    rc = crux_fill_gae_rows(buf, critic, lambda, gamma, first, n, rows_per_env, close_last); if (rc) return rc; }
  if (has_col(buf, CRUX_COL_RETURN)) { rc = crux_fill_returns_rows(buf, gamma, first, n, rows_per_env, close_last); if (rc) return rc; }
  if (nominal && has_col(buf, CRUX_COL_IMPORTANCE_WEIGHT)) {      // step! wrote exp(logpdf(pa, s, a) - logprob) per row (sampler.jl:108-111): the same on the pushed rows (a wrapped block takes two ranges)
    const int64_t n1 = n < buf->capacity - first ? n : buf->capacity - first;
    rc = crux_importance_weight_rows(buf, nominal, nominal_head, first, n1); if (rc) return rc;
    if (n1 < n) { rc = crux_importance_weight_rows(buf, nominal, nominal_head, 0, n - n1); if (rc) return rc; } }
  rc = crux_fill_importance_weights_rows(buf, first, n, rows_per_env, close_last); if (rc) return rc;
  if (has_col(buf, CRUX_COL_COST_ADVANTAGE)) {
    rc = crux_fill_gae_rows_keys(buf, cost_critic, lambda, gamma, first, n, rows_per_env, close_last, CRUX_COL_COST, CRUX_COL_COST_ADVANTAGE); if (rc) return rc; }
  if (has_col(buf, CRUX_COL_COST_RETURN)) { rc = crux_fill_returns_rows_keys(buf, gamma, first, n, rows_per_env, close_last, CRUX_COL_COST, CRUX_COL_COST_RETURN); if (rc) return rc; }
  return CRUX_OK;
}

// steps! for n independent samplers of equal shape in ONE launch (multi-seed runs): problem r rolls out its own policy on its own environments into its own buffer
int32_t crux_rollout_multi(int32_t n, crux_env* const* envs, crux_mlp* const* policies, const crux_rollout_cfg* cfg, crux_buffer* const* bufs, int64_t T, double* sum_r, int64_t* n_episode_end) {
  if (n < 1 || !envs || !policies || !cfg || !bufs || T < 1) return CRUX_EINVAL;
  for (int i = 0; i < n; ++i) CRUX_PLAIN_ONLY("crux_rollout_multi", policies[i]);
  crux_ctx* c = envs[0]->ctx; crux_env* e0 = envs[0]; const NetDesc& pn = policies[0]->nd;
  if (!is_h64(pn) || policies[0]->sigma_head) return crux_fail(c, CRUX_EUNSUP, "steps! (multi): only the 64-wide register-resident rollout kernel is batched");
  std::vector<RolloutArgs> as((size_t)n);
  for (int i = 0; i < n; ++i) {
    crux_env* e = envs[i]; crux_buffer* b = bufs[i]; crux_mlp* p = policies[i];
    if (!e || !b || !p || e->kind != e0->kind || e->n_envs != e0->n_envs || p->nd.n_params != pn.n_params || b->obs_dim != e->obs_dim || b->act_dim != e->act_dim || (int64_t)e->n_envs * T > b->capacity)
      return crux_fail(c, CRUX_EINVAL, "steps! (multi): problem %d does not match problem 0 or its buffer is too small", i);
    fill_rollout_args(as[(size_t)i], e, p, cfg, b, T);
  }
  const size_t bytes = sizeof(RolloutArgs) * (size_t)n;
  RolloutArgs* d_args = (RolloutArgs*)crux_scratch(c, bytes + 256); if (!d_args) return crux_fail(c, CRUX_ENOMEM, "steps! (multi): scratch");
  HIPCHK(c, hipMemcpyAsync(d_args, as.data(), bytes, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  crux_prof_begin(c, CRUX_PROF_ROLLOUT);
  const bool done = launch_rollout_h64(pn, e0->kind, dim3((unsigned)((size_t)n * (size_t)e0->n_envs)), c->stream, as[0], d_args);
  crux_prof_end(c, CRUX_PROF_ROLLOUT);
  if (!done) return crux_fail(c, CRUX_EUNSUP, "steps! (multi): no batched rollout kernel for this policy / environment");
  int32_t rc = crux_launch_check(c, "k_rollout_h64 (multi)"); if (rc) return rc;
  for (int i = 0; i < n; ++i) { if (bufs[i]->prioritized) return crux_fail(c, CRUX_EUNSUP, "steps! (multi): prioritized buffers are not batched"); crux_buffer_ring_advance(bufs[i], (int64_t)envs[i]->n_envs * T); }
  if (sum_r || n_episode_end) {     // n small copies enqueued on the library's stream (never the null stream), one synchronisation
    const size_t per = 2 * (size_t)e0->n_envs; std::vector<double> acc(per * (size_t)n);
    for (int i = 0; i < n; ++i) HIPCHK(c, hipMemcpyAsync(acc.data() + per * (size_t)i, envs[i]->acc, 8 * per, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) rollout_acc_sum(acc.data() + per * (size_t)i, e0->n_envs, sum_r ? sum_r + i : nullptr, n_episode_end ? n_episode_end + i : nullptr);
  }
  return CRUX_OK;
}

int32_t crux_env_step_host(crux_ctx* c, int32_t kind, int64_t n, const double* state, const void* action, const double* uniforms, double* next_state,
                           float* obs, float* r, uint8_t* done) {
  if (!c || n < 0 || !state || !action) return CRUX_EINVAL;
  if (kind != CRUX_ENV_CARTPOLE && kind != CRUX_ENV_PENDULUM && kind != CRUX_ENV_GRIDWORLD) return crux_fail(c, CRUX_EUNSUP, "env kind %d has no device dynamics yet", kind);
  if (n == 0) return CRUX_OK;
  int od, ad, sd; env_dims(kind, 0, 0, &od, &ad, &sd);
  const size_t ab = kind == CRUX_ENV_CARTPOLE ? 2 * (size_t)n : 4 * (size_t)n;     // 2 / 4 one-hot bytes, or one Float32
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t o_s = 0, o_a = o_s + al(8 * (size_t)n * sd), o_ns = o_a + al(ab), o_o = o_ns + al(8 * (size_t)n * sd), o_r = o_o + al(4 * (size_t)n * od), o_d = o_r + al(4 * (size_t)n),
               o_u = o_d + al((size_t)n);
  char* sc = (char*)crux_scratch(c, o_u + al(8 * (size_t)n));
  if (!sc) return crux_fail(c, CRUX_ENOMEM, "env_step: scratch");
  HIPCHK(c, hipMemcpyAsync(sc + o_s, state, 8 * (size_t)n * sd, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(sc + o_a, action, ab, hipMemcpyHostToDevice, c->stream));
  if (uniforms) HIPCHK(c, hipMemcpyAsync(sc + o_u, uniforms, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_env_step, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, kind, n, (const double*)(sc + o_s), (const void*)(sc + o_a),
                     uniforms ? (const double*)(sc + o_u) : (const double*)nullptr, (double*)(sc + o_ns), (float*)(sc + o_o), (float*)(sc + o_r), (uint8_t*)(sc + o_d));
  int32_t rc = crux_launch_check(c, "k_env_step"); if (rc) return rc;
  if (next_state) HIPCHK(c, hipMemcpyAsync(next_state, sc + o_ns, 8 * (size_t)n * sd, hipMemcpyDeviceToHost, c->stream));
  if (obs) HIPCHK(c, hipMemcpyAsync(obs, sc + o_o, 4 * (size_t)n * od, hipMemcpyDeviceToHost, c->stream));
  if (r) HIPCHK(c, hipMemcpyAsync(r, sc + o_r, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (done) HIPCHK(c, hipMemcpyAsync(done, sc + o_d, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CRUX_OK;
}

}  // extern "C"
