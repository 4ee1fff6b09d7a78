// small_solve.hip -- solve(::OffPolicySolver) for a small DQN as one launch: k_dqn_small_solve (one workgroup), k_dqn_tiny_solve (one wave), crux_dqn_small_solve.
#include "train_generic.h"
#include "mlp_forward.h"
#include "ops_small.h"
#include "rollout.h"
void crux_buffer_ring_advance(crux_buffer* b, int64_t N);      // buffer.hip
// ---- the whole off-policy solve loop of a small network in ONE launch ------------------------------------------------------------------------
// solve(::OffPolicySolver) (src/model_free/off_policy.jl:133-147) for the DQN family on networks that fit one workgroup (the README example: DQN on
// SimpleGridWorld, 2-8-4, dN = 4, B = 128): per iteration steps!(dN) -> dN epochs of {rand! (uniform) -> dqn_target -> train!(td_loss)} ->
// polyak_average!. Launched piece by piece this is ~10 kernels and several host round trips per gradient step for a few hundred flops of work. Here
// one workgroup runs `iters` iterations back to back: wave e steps environment e (the generic rollout body, rollout.h), then all four waves run the epochs
// (the uniform draw and gather, the target network through mlp_forward_run, the step through train_generic_run -- the bodies the separate calls
// use, so the results are the same bits), then the target update. Per-epoch info rows are left in device memory for the host to average.
struct SmallSolveArgs {
  RolloutArgs ro;                 // steps! of dN transitions per iteration into the replay ring (base / cfg.i0 advance in the kernel)
  TrainArgs tr;                   // train!(pi, td_loss) on the B rows of the staging buffer (explicit rows 0..B-1)
  NetDesc ndt; float* pt;         // pi_minus
  // staging buffer <- replay buffer gather table (rand!: push!(target, source, ids))
  void* gdst[CRUX_NCOLS]; const void* gsrc[CRUX_NCOLS]; int32_t gre[CRUX_NCOLS]; int32_t gesz[CRUX_NCOLS]; int32_t gn;
  const float* bSP; const float* bR; const uint8_t* bD;     // staging columns the target reads
  int64_t* bidx;                  // staging buffer's indices (device)
  float* qtmp; float* y;          // [nout x B], [B]
  int64_t elements, next, C;      // replay ring state at the first iteration
  int32_t B, epochs, iters, dN, E;
  float gamma, tau;
  uint64_t sample_seed; uint32_t sample_stream; uint64_t i0;
  float* infos;                   // [iters x epochs x 4]: loss, grad norm, Qavg, status
  int32_t* status;
  int32_t lds_train, lds_fwd;     // floats
};
__global__ __launch_bounds__(256) void k_dqn_small_solve(SmallSolveArgs q) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[4];
  __shared__ int32_t st_s[16];
  float* sm_train = sm; float* sm_fwd = sm + q.lds_train; float* sm_ro = sm_fwd + q.lds_fwd;      // rollout: per wave hbuf[2][1024] + misc
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nout = q.ndt.dims[q.ndt.L], npar = q.tr.nd.n_params, B = q.B;
  float* P = q.tr.p; float* G = q.tr.g; float* M = q.tr.m; float* V = q.tr.v; float* PT = q.pt; double* BP = q.tr.bp;
  const float* bS = q.tr.S; const void* bA = q.tr.A; const float* bSP = q.bSP; const float* bR = q.bR; const uint8_t* bD = q.bD; float* Y = q.y; float* QT = q.qtmp; const int32_t* IDS = q.tr.ids;
  if (tid < 16) st_s[tid] = 0;
  __syncthreads();
  int64_t elements = q.elements, next = q.next; int err = 0;
  unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl = __builtin_amdgcn_s_memtime();
#define SS_T(k_) do { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); tacc[k_] += tn_ - tl; tl = tn_; } while (0)
  for (int it = 0; it < q.iters && !err; ++it) {
    const uint64_t si = q.i0 + (uint64_t)it * (uint64_t)q.dN;             // S.i of this iteration (off_policy.jl:134)
    // ---- steps!(sampler, buffer, Nsteps = dN, explore = true, i = S.i) (:138)
    if (wv < q.E) { RolloutArgs ro = q.ro; ro.base = next; ro.cfg.i0 = si; ro.p = P;
      rollout_generic_wave(ro, wv, lane, (float (*)[1024])(sm_ro + (size_t)wv * (2 * 1024 + ENV_MAXOBS + 8)), sm_ro + (size_t)wv * (2 * 1024 + ENV_MAXOBS + 8) + 2 * 1024); }
    next = (next + q.dN) % q.C; elements = elements + q.dN < q.C ? elements + q.dN : q.C;
    __threadfence_block(); __syncthreads(); SS_T(0);
    // ---- value_training (:66-111)
    for (int ep = 0; ep < q.epochs; ++ep) {
      const uint64_t ictr = si * (uint64_t)q.epochs + (uint64_t)ep;
      // rand!(D, buffer): uniform_sample! (experience_buffer.jl:317-321) with the library's Philox draw (per.hip UniformIdsOp), then the row gather
      for (int j = tid; j < B; j += 256) { const crux_u32x4 x = crux_philox(q.sample_seed, ictr * (uint64_t)B + (uint64_t)j, q.sample_stream, CRUX_RNG_SAMPLE);
        q.bidx[j] = (int64_t)(((uint64_t)x.v[0] * (uint64_t)elements) >> 32); }
      __threadfence_block(); __syncthreads(); SS_T(1);
      for (int k = 0; k < q.gn; ++k) { const int re = q.gre[k];
        for (int t = tid; t < B * re; t += 256) { const int j = t / re, e2 = t - j * re; const int64_t sidx = q.bidx[j] * re + e2;
          if (q.gesz[k] == 4) ((uint32_t*)q.gdst[k])[t] = ((const uint32_t*)q.gsrc[k])[sidx];
          else ((uint8_t*)q.gdst[k])[t] = ((const uint8_t*)q.gsrc[k])[sidx]; } }
      __threadfence_block(); __syncthreads(); SS_T(2);
      // y = dqn_target(pi_minus, D) (dqn.jl:4-6)
      mlp_forward_run(q.ndt, PT, bSP, B, QT, sm_fwd, 0u, 1u);
      __threadfence_block(); __syncthreads();
      for (unsigned b = 0; b * 256u < (unsigned)B; ++b) DqnTargetOp::run(b, 1u, QT, nout, bR, bD, q.gamma, (int64_t)B, Y);
      __threadfence_block(); __syncthreads(); SS_T(3);
      // train!(pi, td_loss) (training.jl:13-25)
      { TrainArgs tr = q.tr; tr.p = P; tr.g = G; tr.m = M; tr.v = V; tr.bp = BP; tr.S = bS; tr.A = bA; tr.Y = Y; tr.ids = IDS; tr.status = st_s;
        tr.epoch_infos = q.infos + ((size_t)it * q.epochs + ep) * CRUX_INFO_N; train_generic_run(tr, sm_train, red); }
      __threadfence_block(); __syncthreads(); SS_T(4);
      if (st_s[0] != 0) { err = st_s[0]; break; }
    }
    if (err) break;
    // target_update: polyak_average!(pi_minus, pi, tau) (:108, policies.jl:48-59)
    { const float omt = __fsub_rn(1.0f, q.tau);
      for (int i = tid; i < npar; i += 256) PT[i] = __fadd_rn(__fmul_rn(q.tau, P[i]), __fmul_rn(omt, PT[i])); }
    __threadfence_block(); __syncthreads();
  }
  if (tid == 0) { q.status[0] = st_s[0]; q.status[8] = err; for (int z = 0; z < 8; ++z) ((unsigned long long*)(q.status + 16))[z] = tacc[z]; }
}

typedef float f32x4_env __attribute__((ext_vector_type(4)));
// ---- the same solve loop for a TINY network, wave-resident ----------------------------------------------------------------------------------
// The README example's DQN (SimpleGridWorld, 2 -> 8 -> 4, 60 parameters, B = 128) is a few hundred flops per gradient step: in k_dqn_small_solve the step
// still cost 68 us, almost all of it workgroup barriers and Float64 block reductions of the shape-generic learner body -- one host core does the step in
// 21 us. Here ONE wave owns the whole problem: parameter i, its Adam moments and the target network's copy live in lane i's registers and are broadcast with
// v_readlane; the replay ring is mirrored in LDS (the rollout body still writes the global columns, the new rows are copied over after each steps!);
// lane j evaluates samples j and j + 64 of the minibatch (target network, Q network, td_loss and the per-sample parameter gradients in registers), the
// 60 x 64 partial gradients are transposed through LDS so that lane i adds parameter i's contributions in lane order, and applies Flux's Adam (Float64 per
// element, like the generic body). No workgroup barrier exists in the loop. Same mathematics as the call-by-call loop with a different (fixed) summation
// order of the minibatch gradient: parity against the oracle is to float tolerance (tests/test_gpu_components.py: the solve loop keeps the oracle's
// trajectories and replay contents exactly, the networks to 1e-5), not bit-identity with k_dqn_small_solve, which stays as the shape-generic form.
template <int IN, int H, int OUT>
__global__ __launch_bounds__(64) void k_dqn_tiny_solve(SmallSolveArgs q) {
  constexpr int NP = H * IN + H + OUT * H + OUT, oW1 = 0, oB1 = H * IN, oW2 = oB1 + H, oB2 = oW2 + OUT * H;
  static_assert(NP <= 64 && OUT == 4, "one parameter per lane; the one-hot action row is read as one 32-bit word");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x; const int B = q.B; const int64_t C = q.C;
  float* sm_ro = sm;                                                   // rollout body: hbuf[2][1024] + misc
  float* mS = sm_ro + (2 * 1024 + ENV_MAXOBS + 8);                     // ring mirror: S [C x IN], SP [C x IN], R [C], A (action index) [C], D [C]
  float* mSP = mS + C * IN; float* mR = mSP + C * IN; int32_t* mA = (int32_t*)(mR + C); int32_t* mD = mA + C;
  float* red = (float*)(mD + C);                                       // [NP][64] transpose buffer
  const float* gS = q.ro.S; const float* gSP = q.ro.SP; const float* gR = q.ro.R; const uint8_t* gA = (const uint8_t*)q.ro.A; const uint8_t* gD = q.ro.D;
  auto mirror_row = [&](int64_t row) {
    for (int k = 0; k < IN; ++k) { mS[row * IN + k] = gS[row * IN + k]; mSP[row * IN + k] = gSP[row * IN + k]; }
    mR[row] = gR[row]; int ai = 0; for (int k = 0; k < OUT; ++k) ai = gA[row * OUT + k] ? k : ai; mA[row] = ai; mD[row] = gD[row] ? 1 : 0;
  };
  for (int64_t row = lane; row < q.elements; row += 64) mirror_row(row);
  __shared__ float th_s[64]; __shared__ double st_s[ENV_MAXSD]; __shared__ int64_t cnt_s[3]; __shared__ float sv_s[ENV_MAXOBS]; __shared__ double acc_s[2];
  if (lane == 0) { for (int i = 0; i < q.ro.sd; ++i) st_s[i] = q.ro.state[i];
    cnt_s[0] = q.ro.ep_len[0]; cnt_s[1] = q.ro.n_resets[0]; cnt_s[2] = q.ro.steps_taken[0]; acc_s[0] = q.ro.acc[0]; acc_s[1] = q.ro.acc[1]; }
  if (lane < q.ro.od) sv_s[lane] = q.ro.svec[lane];
  float p = lane < NP ? q.tr.p[lane] : 0.f, pt = lane < NP ? q.pt[lane] : 0.f, am = lane < NP ? q.tr.m[lane] : 0.f, av = lane < NP ? q.tr.v[lane] : 0.f;
  double bp1 = q.tr.bp[0], bp2 = q.tr.bp[1];
  int64_t elements = q.elements, next = q.next; int err = 0;
  const float invB = 1.0f / (float)B;
  auto W = [&](float reg, int i) -> float { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, reg), i)); };   // parameter i, wave-uniform
  auto forward = [&](float reg, const float (&x)[IN], float (&h)[H], float (&o)[OUT]) {
#pragma unroll
    for (int j = 0; j < H; ++j) { float acc = 0.f;
#pragma unroll
      for (int k = 0; k < IN; ++k) acc = fmaf(W(reg, oW1 + j + H * k), x[k], acc);
      const float z = acc + W(reg, oB1 + j); h[j] = z > 0.f ? z : 0.f; }
#pragma unroll
    for (int j = 0; j < OUT; ++j) { float acc = 0.f;
#pragma unroll
      for (int k = 0; k < H; ++k) acc = fmaf(W(reg, oW2 + j + OUT * k), h[k], acc);
      o[j] = acc + W(reg, oB2 + j); }
  };
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
  const bool grid = q.ro.kind == CRUX_ENV_GRIDWORLD && q.ro.od == IN && q.ro.ad == OUT;
  double gst[ENV_MAXSD]; float gx[IN]; int64_t g_ep_len = cnt_s[0], g_n_resets = cnt_s[1], g_steps_taken = cnt_s[2], g_nee = 0; double g_sum_r = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i) gst[i] = st_s[i];
#pragma unroll
  for (int k = 0; k < IN; ++k) gx[k] = sv_s[k];
  unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl = __builtin_amdgcn_s_memtime();      // phase shares (CRUX_SMALL_SOLVE_TIMING): rollout | sample + forward / backward | transpose-reduce | statistics + Adam
#define TS_T(k_) do { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); tacc[k_] += tn_ - tl; tl = tn_; } while (0)
  for (int it = 0; it < q.iters && !err; ++it) {
    const uint64_t si = q.i0 + (uint64_t)it * (uint64_t)q.dN;
    // ---- steps!(sampler, buffer, Nsteps = dN, explore = true, i = S.i): the generic rollout body, with theta and the sampler's state (env state, episode
    // counters, current observation) pointed at LDS copies -- read from global memory they cost a dependent L2 round trip per layer and per call (the rollout was
    // 2/3 of the solve); the buffer columns it writes stay in global memory, where the call-by-call loop leaves them
    if (grid) {
      // SimpleGridWorld (the README example): the whole sampler lives in registers, every lane carrying an identical copy like the 64-wide rollout kernel does. The
      // policy forward reads theta from the lane registers (the arithmetic order of the generic body: fma over k ascending, + bias, relu), and the tail runs with
      // compile-time environment kind and dimensions, so that its per-step arrays are registers -- called with run-time dimensions they are private memory and
      // a step cost 7.4 us (2/3 of the whole solve).
      RolloutArgs ro = q.ro; ro.base = next; ro.cfg.i0 = si; g_sum_r = 0.0; g_nee = 0;
      for (int64_t t = 0; t < ro.T; ++t) {
        const int64_t j = (ro.base + t) % ro.C;
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < IN; ++k) ro.S[(size_t)j * IN + k] = gx[k]; }
        float h[H], z[OUT]; forward(p, gx, h, z);
        float nx[ENV_MAXOBS];
        rollout_tail(ro, z, IN, OUT, OUT, CRUX_ENV_GRIDWORLD, 0, t, j, lane == 0, gst, g_ep_len, g_n_resets, g_steps_taken, g_sum_r, g_nee, nx);
#pragma unroll
        for (int k = 0; k < IN; ++k) gx[k] = nx[k];
      }
    } else {
    if (lane < NP) th_s[lane] = p;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
    { RolloutArgs ro = q.ro; ro.base = next; ro.cfg.i0 = si;
      ro.p = th_s; ro.state = st_s; ro.ep_len = &cnt_s[0]; ro.n_resets = &cnt_s[1]; ro.steps_taken = &cnt_s[2]; ro.svec = sv_s; ro.acc = acc_s;
      rollout_generic_wave(ro, 0, lane, (float (*)[1024])sm_ro, sm_ro + 2 * 1024); }
    }
    TS_T(5);
    __threadfence();
    if (lane < q.dN) mirror_row((next + lane) % C);
    next = (next + q.dN) % C; elements = elements + q.dN < C ? elements + q.dN : C;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
    TS_T(0);
    for (int ep = 0; ep < q.epochs; ++ep) {
      const uint64_t ictr = si * (uint64_t)q.epochs + (uint64_t)ep;
      float g[NP];
#pragma unroll
      for (int k = 0; k < NP; ++k) g[k] = 0.f;
      double s_sq = 0.0, s_q = 0.0;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int j = lane + 64 * half;
        if (j < B) {
          // rand!(D, buffer): uniform_sample! with the library's Philox draw (per.hip UniformIdsOp)
          const crux_u32x4 xr = crux_philox(q.sample_seed, ictr * (uint64_t)B + (uint64_t)j, q.sample_stream, CRUX_RNG_SAMPLE);
          const int64_t row = (int64_t)(((uint64_t)xr.v[0] * (uint64_t)elements) >> 32);
          q.bidx[j] = row;
          float x[IN], xp[IN];
#pragma unroll
          for (int k = 0; k < IN; ++k) { x[k] = mS[row * IN + k]; xp[k] = mSP[row * IN + k]; }
          const float r = mR[row]; const int ai = mA[row]; const float nd = 1.f - (mD[row] ? 1.f : 0.f);
          // y = dqn_target(pi_minus, D) (dqn.jl:4-6): r + gamma (1 - done) max_a Q-(sp, a), un-fused
          float h[H], o[OUT]; forward(pt, xp, h, o);
          float mx = o[0];
#pragma unroll
          for (int k = 1; k < OUT; ++k) mx = o[k] > mx ? o[k] : mx;
          const float gn = q.gamma * nd; const float tt = gn * mx; const float y = r + tt;
          // td_loss (utils.jl:76-87): mean((Q(s, a) - y)^2) and its pullback
          forward(p, x, h, o);
          float Q = 0.f;
#pragma unroll
          for (int k = 0; k < OUT; ++k) Q += o[k] * (k == ai ? 1.f : 0.f);
          const float d = Q - y; s_sq += (double)(d * d); s_q += (double)Q;
          float dq[OUT], dh[H];
#pragma unroll
          for (int k = 0; k < OUT; ++k) dq[k] = (k == ai) ? 2.f * d * 1.f * invB : 0.f;
#pragma unroll
          for (int k = 0; k < H; ++k) { float acc = 0.f;
#pragma unroll
            for (int oo = 0; oo < OUT; ++oo) { g[oW2 + oo + OUT * k] = fmaf(dq[oo], h[k], g[oW2 + oo + OUT * k]); acc = fmaf(W(p, oW2 + oo + OUT * k), dq[oo], acc); }
            dh[k] = h[k] > 0.f ? acc : 0.f; }                                                                   // relu'(0) = 0
#pragma unroll
          for (int oo = 0; oo < OUT; ++oo) g[oB2 + oo] += dq[oo];
#pragma unroll
          for (int k = 0; k < IN; ++k)
#pragma unroll
            for (int oo = 0; oo < H; ++oo) g[oW1 + oo + H * k] = fmaf(dh[oo], x[k], g[oW1 + oo + H * k]);
#pragma unroll
          for (int oo = 0; oo < H; ++oo) g[oB1 + oo] += dh[oo];
        }
      }
      TS_T(1);
      // transpose: lane i adds parameter i's 64 partials in lane order
#pragma unroll
      for (int k = 0; k < NP; ++k) red[k * 64 + lane] = g[k];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
      float gi = 0.f;
      if (lane < NP) {
#pragma unroll
        for (int l4 = 0; l4 < 16; ++l4) { const f32x4_env v4 = *(const f32x4_env*)&red[lane * 64 + 4 * l4]; gi = ((((gi + v4[0]) + v4[1]) + v4[2]) + v4[3]); } }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
      TS_T(2);
      const double t_ssq = wave_sum_d(lane < NP ? (double)gi * (double)gi : 0.0), t_sq = wave_sum_d(s_sq), t_q = wave_sum_d(s_q);
      const float gnorm = (float)sqrt(t_ssq);
      if (lane == 0) { float* e = q.infos + ((size_t)it * q.epochs + ep) * CRUX_INFO_N;
        e[CRUX_INFO_LOSS] = (float)(t_sq / (double)B); e[CRUX_INFO_GRAD_NORM] = gnorm; e[2] = (float)(t_q / (double)B); }
      if (isnan(gnorm)) { err = CRUX_ENAN; break; }                                                               // training.jl:20 -- no update
      if (lane < NP) {   // Flux.update!(Adam) (training.jl:21), Float64 per element like the reference
        const double gd = (double)gi; const double b1 = q.tr.b1, b2 = q.tr.b2;
        const float mi = (float)(b1 * (double)am + (1.0 - b1) * gd);
        const float vi = (float)(b2 * (double)av + ((1.0 - b2) * gd) * gd);
        const float dd = (float)((double)mi / (1.0 - bp1) / (sqrt((double)vi / (1.0 - bp2)) + q.tr.eps) * q.tr.eta);
        am = mi; av = vi; p = p - dd; }
      bp1 *= q.tr.b1; bp2 *= q.tr.b2;
      TS_T(4);
    }
    if (err) break;
    { const float omt = __fsub_rn(1.0f, q.tau); pt = __fadd_rn(__fmul_rn(q.tau, p), __fmul_rn(omt, pt)); }          // polyak_average!(pi_minus, pi, tau) (:108)
  }
  // ---- leave everything where the call-by-call loop leaves it: networks, Adam state, and the staging batch = the last minibatch drawn
  if (lane < NP) { q.tr.p[lane] = p; q.pt[lane] = pt; q.tr.m[lane] = am; q.tr.v[lane] = av; q.tr.g[lane] = 0.f; }
  if (grid && lane == 0) { st_s[0] = gst[0]; st_s[1] = gst[1]; cnt_s[0] = g_ep_len; cnt_s[1] = g_n_resets; cnt_s[2] = g_steps_taken; acc_s[0] = g_sum_r; acc_s[1] = (double)g_nee;
#pragma unroll
    for (int k = 0; k < IN; ++k) sv_s[k] = gx[k]; }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
  if (lane == 0) { for (int i = 0; i < q.ro.sd; ++i) q.ro.state[i] = st_s[i];           // the sampler's state back where the call-by-call loop keeps it
    q.ro.ep_len[0] = cnt_s[0]; q.ro.n_resets[0] = cnt_s[1]; q.ro.steps_taken[0] = cnt_s[2]; q.ro.acc[0] = acc_s[0]; q.ro.acc[1] = acc_s[1]; }
  if (lane < q.ro.od) q.ro.svec[lane] = sv_s[lane];
  __threadfence();
  for (int k = 0; k < q.gn; ++k) { const int re = q.gre[k];
    for (int t = lane; t < B * re; t += 64) { const int j = t / re, e2 = t - j * re; const int64_t sidx = q.bidx[j] * re + e2;
      if (q.gesz[k] == 4) ((uint32_t*)q.gdst[k])[t] = ((const uint32_t*)q.gsrc[k])[sidx];
      else ((uint8_t*)q.gdst[k])[t] = ((const uint8_t*)q.gsrc[k])[sidx]; } }
  if (lane == 0) { q.tr.bp[0] = bp1; q.tr.bp[1] = bp2; q.status[0] = err; q.status[8] = err; for (int z = 0; z < 8; ++z) ((unsigned long long*)(q.status + 16))[z] = tacc[z]; }
}

// solve(::OffPolicySolver) for a small DQN (see k_dqn_small_solve). Preconditions (CRUX_EUNSUP otherwise, the caller then loops piece by piece): uniform replay,
// batch capacity == B <= 256, at most 4 environments, dN a multiple of them, both networks narrower than the dense engine's threshold, a rollout that the
// generic kernel would run. infos: host [iters x epochs x CRUX_INFO_N] (loss, grad norm, [2] = Qavg per epoch).
extern "C" int32_t crux_dqn_small_solve(crux_mlp* net, crux_mlp* target_net, crux_env* e, const crux_rollout_cfg* cfg, crux_buffer* source, crux_buffer* batch,
                                        int32_t iters, int32_t dN, int32_t epochs, float gamma, float tau, int32_t use_weight, uint64_t i0, float* infos, double* sum_r, int64_t* n_episode_end) { CRUX_PLAIN_ONLY("crux_dqn_small_solve", net, target_net); CRUX_NO_CLIP("crux_dqn_small_solve", net);
  if (!net || !target_net || !e || !cfg || !source || !batch || iters < 1 || dN < 1 || epochs < 1) return CRUX_EINVAL;
  crux_ctx* c = net->ctx; const int64_t B = batch->capacity; const int E = e->n_envs;
  const NetDesc& pn = net->nd;
  if (source->prioritized || batch->prioritized || B > 256 || B < 1 || E > 4 || dN % E || pn.maxdim >= CRUX_DENSE_MIN_WIDTH || target_net->nd.maxdim >= CRUX_DENSE_MIN_WIDTH || is_h64(pn) ||
      target_net->nd.n_params != pn.n_params || !net->has_adam || cfg->head != CRUX_HEAD_GREEDY_Q || source->act_kind != CRUX_ACTION_DISCRETE || pn.dims[pn.L] != source->act_dim || dN > source->capacity || use_weight)
    return crux_fail(c, CRUX_EUNSUP, "dqn_small_solve: configuration outside the one-launch solve kernel");
  if (source->obs_dim != e->obs_dim || source->act_dim != e->act_dim || batch->obs_dim != source->obs_dim || batch->act_dim != source->act_dim || pn.dims[0] != e->obs_dim) return crux_fail(c, CRUX_EINVAL, "dqn_small_solve: shapes of env / buffers / network differ");
  SmallSolveArgs q{};
  fill_rollout_args(q.ro, e, net, cfg, source, dN / E);
  // train!(pi, td_loss) on rows 0..B-1 of the staging buffer (the ids live in the staging buffer's order scratch)
  TrainArgs& a = q.tr; memset(&a, 0, sizeof a);
  train_args_net(a, net);
  a.S = (const float*)batch->col[CRUX_COL_S]; a.A = batch->col[CRUX_COL_A]; a.od = batch->obs_dim; a.ad = batch->act_dim; a.act_kind = batch->act_kind;
  a.loss = CRUX_LOSS_TD_INTERNAL; a.head = CRUX_HEAD_GREEDY_Q; a.bs = (int32_t)B; a.epochs = 1; a.max_batches = 0; a.target_kl = -1.f; a.len = B; a.apply = 1;
  a.order_a = batch->order_a; a.order_b = batch->order_b;
  const size_t nout = (size_t)pn.dims[pn.L];
  const size_t small = 4 * ((size_t)B * nout + (size_t)B) + 4 * (size_t)B + 2048;
  char* sc = (char*)crux_scratch(c, small + sizeof(float) * CRUX_INFO_N * (size_t)iters * (size_t)epochs + 4096); if (!sc) return crux_fail(c, CRUX_ENOMEM, "dqn_small_solve: scratch");
  int32_t* d_ids = (int32_t*)sc; q.qtmp = (float*)(sc + ((4 * (size_t)B + 255) / 256) * 256); q.y = q.qtmp + B * nout; q.status = (int32_t*)(q.y + B); q.infos = (float*)(sc + ((small + 255) / 256) * 256);
  { std::vector<int32_t> h((size_t)B); for (int64_t j = 0; j < B; ++j) h[(size_t)j] = (int32_t)j;
    HIPCHK(c, hipMemcpyAsync(d_ids, h.data(), 4 * (size_t)B, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipMemsetAsync(q.status, 0, 256, c->stream));
    HIPCHK(c, hipMemsetAsync(q.infos, 0, sizeof(float) * CRUX_INFO_N * (size_t)iters * (size_t)epochs, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
  a.ids = d_ids; a.n_ids = B; a.Y = q.y; a.Wt = nullptr; a.status = q.status;
  q.ndt = target_net->nd; q.pt = target_net->p;
  q.gn = 0; for (int k = 0; k < CRUX_NCOLS; ++k) { if (!has_col(batch, k) || !has_col(source, k)) continue; const size_t st = col_stride(batch, k); const int z = q.gn++;
    q.gdst[z] = batch->col[k]; q.gsrc[z] = source->col[k]; q.gesz[z] = st % 4 == 0 ? 4 : 1; q.gre[z] = (int32_t)(st % 4 == 0 ? st / 4 : st);
  }
  q.bSP = (const float*)batch->col[CRUX_COL_SP]; q.bR = (const float*)batch->col[CRUX_COL_R]; q.bD = (const uint8_t*)batch->col[CRUX_COL_DONE]; q.bidx = batch->d_indices;
  q.elements = source->elements; q.next = source->next_ind; q.C = source->capacity; q.B = (int32_t)B; q.epochs = epochs; q.iters = iters; q.dN = dN; q.E = E;
  q.gamma = gamma; q.tau = tau; q.sample_seed = source->sample_seed; q.sample_stream = source->sample_stream; q.i0 = i0;
  q.lds_train = (int32_t)((generic_lds_bytes(pn) / sizeof(float) + 63) / 64 * 64); q.lds_fwd = (int32_t)(2 * (size_t)target_net->nd.maxdim * FWD_TS);
  size_t lds = sizeof(float) * ((size_t)q.lds_train + (size_t)q.lds_fwd + (size_t)E * (2 * 1024 + ENV_MAXOBS + 8));
  if (lds > 150 * 1024) return crux_fail(c, CRUX_EUNSUP, "dqn_small_solve: %zu bytes of LDS", lds);
  // the README shape (2 -> 8 -> 4, relu, one environment, B <= 128) with a ring that fits LDS: the wave-resident kernel
  const size_t tiny_lds = sizeof(float) * ((size_t)(2 * 1024 + ENV_MAXOBS + 8) + (size_t)source->capacity * (2 * 2 + 3) + 60 * 64) + 64;
  const bool tiny = pn.L == 2 && pn.dims[0] == 2 && pn.dims[1] == 8 && pn.dims[2] == 4 && pn.acts[0] == CRUX_ACT_RELU && pn.acts[1] == CRUX_ACT_IDENTITY && pn.n_extra == 0 &&
                    target_net->nd.L == 2 && target_net->nd.dims[1] == 8 && target_net->nd.acts[0] == CRUX_ACT_RELU && E == 1 && B <= 128 && dN <= 64 && tiny_lds <= 60 * 1024 &&
                    !crux_sw().small_solve_generic;
  crux_prof_begin(c, tiny ? CRUX_PROF_TINY_SOLVE : CRUX_PROF_TD_STEP);
  if (tiny) hipLaunchKernelGGL((k_dqn_tiny_solve<2, 8, 4>), dim3(1), dim3(64), tiny_lds, c->stream, q);
  else {
    static size_t attr_set = 0;
    if (lds > attr_set) { HIPCHK(c, hipFuncSetAttribute((const void*)k_dqn_small_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr_set = lds; }
    hipLaunchKernelGGL(k_dqn_small_solve, dim3(1), dim3(256), lds, c->stream, q);
  }
  crux_prof_end(c, tiny ? CRUX_PROF_TINY_SOLVE : CRUX_PROF_TD_STEP);
  int32_t rc = crux_launch_check(c, "k_dqn_small_solve"); if (rc) return rc;
  int32_t hst9[9] = {0}; int32_t hst[2];
  HIPCHK(c, hipMemcpyAsync(hst9, q.status, sizeof hst9, hipMemcpyDeviceToHost, c->stream));
  if (infos) HIPCHK(c, hipMemcpyAsync(infos, q.infos, sizeof(float) * CRUX_INFO_N * (size_t)iters * (size_t)epochs, hipMemcpyDeviceToHost, c->stream));
  std::vector<double> acc(2 * (size_t)E);
  HIPCHK(c, hipMemcpyAsync(acc.data(), e->acc, 16 * (size_t)E, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // host-side bookkeeping of the rings (push!, experience_buffer.jl:256-257) and of the staging buffer's sample state
  for (int it = 0; it < iters; ++it) crux_buffer_ring_advance(source, dN);
  batch->elements = B; batch->next_ind = 0; batch->total_count += (int64_t)B * epochs * iters; batch->indices_n = B; batch->indices_stale = true;
  rollout_acc_sum(acc.data(), E, sum_r, n_episode_end);
  hst[0] = hst9[0]; hst[1] = hst9[8];
  if (crux_sw().small_solve_timing) { unsigned long long tt[8]; (void)hipMemcpy(tt, q.status + 16, sizeof tt, hipMemcpyDeviceToHost); unsigned long long tot = 0; for (auto v : tt) tot += v;
    fprintf(stderr, "[small-solve] rollout %.1f%% ids (tiny kernel: sample + forward / backward) %.1f%% gather (tiny: transpose-reduce) %.1f%% target %.1f%% train (tiny: statistics + Adam) %.1f%%\n", 100.0 * tt[0] / tot, 100.0 * tt[1] / tot, 100.0 * tt[2] / tot, 100.0 * tt[3] / tot, 100.0 * tt[4] / tot); fprintf(stderr, "[small-solve] tiny: rollout body %.1f%%, fence + mirror %.1f%%\n", 100.0 * tt[5] / tot, 100.0 * tt[0] / tot); }
  if (hst[1] == CRUX_ENAN || hst[0] == CRUX_ENAN) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20)");
  if (hst[1]) return crux_fail(c, hst[1], "small solve kernel reported status %d", hst[1]);
  return CRUX_OK;
}
