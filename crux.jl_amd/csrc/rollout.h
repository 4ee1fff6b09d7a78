// rollout.h -- what env.hip (the rollout and explore kernels) and small_solve.hip (the one-launch DQN solve) share of the Samplers: the environment dynamics, step! after the
// policy forward (rollout_head / rollout_tail), the forward of ONE observation (h64_forward, rollout_generic_forward), the generic rollout body, and the host side's shape table.
#pragma once
#include "common.h"
#define ENV_MAXSD 32          // SYNTH keeps one Float64 per observation; CartPole 4, Pendulum / GridWorld 2
#define ENV_MAXOBS 32
#define PI_D 3.14159265358979323846

// ---- dynamics (float64, same operation order as the oracle) ------------------------------------------
__device__ __forceinline__ void cartpole_step(const double* s, int action, double* sn, float* r, uint8_t* done) {
  const double gravity = 9.8, masscart = 1.0, masspole = 0.1, total_mass = masspole + masscart, length = 0.5,
               polemass_length = masspole * length, force_mag = 10.0, tau = 0.02;
  double x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
  const double force = action == 1 ? force_mag : -force_mag;
  const double costheta = cos(theta), sintheta = sin(theta);
  const double temp = __ddiv_rn(__dadd_rn(force, __dmul_rn(__dmul_rn(polemass_length, __dmul_rn(theta_dot, theta_dot)), sintheta)), total_mass);
  const double den = __dmul_rn(length, __dsub_rn(4.0 / 3.0, __ddiv_rn(__dmul_rn(masspole, __dmul_rn(costheta, costheta)), total_mass)));
  const double thetaacc = __ddiv_rn(__dsub_rn(__dmul_rn(gravity, sintheta), __dmul_rn(costheta, temp)), den);
  const double xacc = __dsub_rn(temp, __ddiv_rn(__dmul_rn(__dmul_rn(polemass_length, thetaacc), costheta), total_mass));
  x = __dadd_rn(x, __dmul_rn(tau, x_dot)); x_dot = __dadd_rn(x_dot, __dmul_rn(tau, xacc));
  theta = __dadd_rn(theta, __dmul_rn(tau, theta_dot)); theta_dot = __dadd_rn(theta_dot, __dmul_rn(tau, thetaacc));
  sn[0] = x; sn[1] = x_dot; sn[2] = theta; sn[3] = theta_dot;
  const double xth = 2.4, thth = 12.0 * 2.0 * PI_D / 360.0;
  *done = (x < -xth || x > xth || theta < -thth || theta > thth) ? 1 : 0;
  *r = 1.0f;
}
__device__ __forceinline__ double angle_normalize(double x) { double t = fmod(x + PI_D, 2.0 * PI_D); if (t < 0) t += 2.0 * PI_D; return t - PI_D; }
__device__ __forceinline__ void pendulum_step(const double* s, float a, double* sn, float* r, uint8_t* done) {
  const double g = 10.0, m = 1.0, l = 1.0, dt = 0.05, max_speed = 8.0, max_torque = 2.0;
  const double th = s[0], thdot = s[1];
  double u = (double)a; if (u < -max_torque) u = -max_torque; if (u > max_torque) u = max_torque;
  const double an = angle_normalize(th);
  const double costs = __dadd_rn(__dadd_rn(__dmul_rn(an, an), __dmul_rn(0.1, __dmul_rn(thdot, thdot))), __dmul_rn(0.001, __dmul_rn(u, u)));
  double newthdot = __dadd_rn(thdot, __dmul_rn(__dadd_rn(__dmul_rn(3.0 * g / (2.0 * l), sin(th)), __dmul_rn(3.0 / (m * l * l), u)), dt));
  if (newthdot < -max_speed) newthdot = -max_speed; if (newthdot > max_speed) newthdot = max_speed;
  sn[0] = __dadd_rn(th, __dmul_rn(newthdot, dt)); sn[1] = newthdot; *r = (float)(-costs); *done = 0;
}
// POMDPModels.SimpleGridWorld restated (README example, configs[0]); see the oracle for the definition.
__device__ __forceinline__ float gridworld_reward(double x, double y) {
  if (x == 4 && y == 3) return -10.f; if (x == 4 && y == 6) return -5.f; if (x == 9 && y == 3) return 10.f; if (x == 8 && y == 8) return 3.f; return 0.f;
}
__device__ __forceinline__ void gridworld_step(const double* s, int a, double u, double* sn, float* r, uint8_t* done) {
  const double tprob = 0.7;
  const double x = s[0], y = s[1];
  const float rw = gridworld_reward(x, y);
  *r = rw;
  if (rw != 0.f) { sn[0] = -1; sn[1] = -1; *done = 1; return; }
  int dir = a;
  if (!(u < tprob)) { int k = (int)((u - tprob) / (1.0 - tprob) * 3.0); if (k > 2) k = 2; int cnt = 0;
    for (int d = 0; d < 4; ++d) { if (d == a) continue; if (cnt == k) { dir = d; break; } ++cnt; } }
  const double ddx = dir == 2 ? -1.0 : (dir == 3 ? 1.0 : 0.0), ddy = dir == 0 ? 1.0 : (dir == 1 ? -1.0 : 0.0);
  double nx = x + ddx, ny = y + ddy;
  if (nx < 1 || nx > 10 || ny < 1 || ny > 10) { nx = x; ny = y; }
  sn[0] = nx; sn[1] = ny; *done = 0;
}
// SYNTH: see include/cruxhip.h for the definition (the oracle's synth_step is the twin)
__device__ __forceinline__ bool env_is_synth(int kind) { return kind == CRUX_ENV_SYNTH || kind == CRUX_ENV_SYNTH_DISCRETE; }
__device__ __forceinline__ void env_writelane(uint32_t& dst, const uint32_t uniform_v, const int l) {      // dst[lane l] = the (wave-uniform) value
  const int sv = __builtin_amdgcn_readfirstlane((int)uniform_v);
  asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(dst) : "s"(sv), "n"(l));
}
__device__ __forceinline__ double env_readlane_f64(const double v, const int l) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// par_lane >= 0: the whole wave executes this with identical arguments in every lane (the register-resident rollout kernels); lane i evaluates element i -- the Float64 sin
// is the cost of the step -- and the elements are collected with v_readlane (so, sa compile-time there). The same operations per element: the same bits.
__device__ __forceinline__ void synth_step(int so, int sa, bool discrete, const double* s, int ai, const float* a, double* sn, float* r, uint8_t* done, const int par_lane = -1) {
  double ss = 0.0;
  if (par_lane >= 0) {
    // lane i takes s[i] and s[i+1] with v_writelane (a select chain over the lane id is turned into an indexed load of the state array, which then lives in scratch)
    uint32_t il = 0, ih = 0, jl = 0, jh = 0; double u = 0.0;
#pragma unroll
    for (int i = 0; i < so; ++i) { const uint64_t bi = __builtin_bit_cast(uint64_t, s[i]), bj = __builtin_bit_cast(uint64_t, s[(i + 1) % so]);
      env_writelane(il, (uint32_t)bi, i); env_writelane(ih, (uint32_t)(bi >> 32), i); env_writelane(jl, (uint32_t)bj, i); env_writelane(jh, (uint32_t)(bj >> 32), i); }
    const double si = __builtin_bit_cast(double, ((uint64_t)ih << 32) | il), sj = __builtin_bit_cast(double, ((uint64_t)jh << 32) | jl);
    const int ii = par_lane < so ? par_lane : 0;
    if (discrete) u = ((ii + ai) % sa == 0) ? 1.0 : -0.25;
    else { float av = a[0];
#pragma unroll
      for (int q = 0; q < sa; ++q) if (ii % sa == q) av = a[q]; u = (double)av; if (u < -1.0) u = -1.0; if (u > 1.0) u = 1.0; }
    const double mine = __dadd_rn(__dmul_rn(0.9, si), __dmul_rn(0.1, sin(__dadd_rn(sj, u))));
#pragma unroll
    for (int i = 0; i < so; ++i) { sn[i] = env_readlane_f64(mine, i); ss = __dadd_rn(ss, __dmul_rn(sn[i], sn[i])); }
  } else
  for (int i = 0; i < so; ++i) {
    double u;
    if (discrete) u = ((i + ai) % sa == 0) ? 1.0 : -0.25;
    else { u = (double)a[i % sa]; if (u < -1.0) u = -1.0; if (u > 1.0) u = 1.0; }
    sn[i] = __dadd_rn(__dmul_rn(0.9, s[i]), __dmul_rn(0.1, sin(__dadd_rn(s[(i + 1) % so], u))));
    ss = __dadd_rn(ss, __dmul_rn(sn[i], sn[i]));
  }
  *r = (float)__dadd_rn(-(ss / (double)so), __dmul_rn(0.05, sn[0]));
  *done = sn[0] > 0.9 ? 1 : 0;
}
// the cost channel of the restated environments (include/cruxhip.h): info["cost"] of the step that reached s' (sampler.jl:65-66,114)
__device__ __forceinline__ float env_cost(int kind, int so, const double* sn) {
  if (env_is_synth(kind)) { const double x = sn[1 % so]; return (float)__dmul_rn(25.0, __dmul_rn(x, x)); }
  if (kind == CRUX_ENV_CARTPOLE) return fabs(sn[2]) > 0.05 ? 1.f : 0.f;
  if (kind == CRUX_ENV_PENDULUM) return fabs(sn[1]) > 4.0 ? 1.f : 0.f;
  return 0.f;
}
__device__ __forceinline__ void env_obs(int kind, const double* s, float* o, int od = 0) {
  if (kind == CRUX_ENV_CARTPOLE) { o[0] = (float)s[0]; o[1] = (float)s[1]; o[2] = (float)s[2]; o[3] = (float)s[3]; }
  else if (kind == CRUX_ENV_PENDULUM) { o[0] = (float)cos(s[0]); o[1] = (float)sin(s[0]); o[2] = (float)s[1]; }
  else if (env_is_synth(kind)) { for (int i = 0; i < od; ++i) o[i] = (float)s[i]; }
  else { o[0] = (float)s[0]; o[1] = (float)s[1]; }
}
__device__ __forceinline__ void env_draw_initial(int kind, uint64_t seed, uint64_t n_resets, uint32_t env, double* s, int sd = 0) {
  if (env_is_synth(kind)) {                                   // U(-0.05, 0.05)^so, two Float64 uniforms per Philox block
    for (int i = 0; i < sd; ++i) { const crux_u32x4 x = crux_philox(seed, 16 * n_resets + (uint64_t)(i >> 1), env, CRUX_RNG_RESET);
      const double ui = (i & 1) ? crux_u32x2_to_f64(x.v[2], x.v[3]) : crux_u32x2_to_f64(x.v[0], x.v[1]); s[i] = __dadd_rn(-0.05, __dmul_rn(0.1, ui)); }
    return;
  }
  const crux_u32x4 a = crux_philox(seed, 2 * n_resets, env, CRUX_RNG_RESET), b = crux_philox(seed, 2 * n_resets + 1, env, CRUX_RNG_RESET);
  const double u0 = crux_u32x2_to_f64(a.v[0], a.v[1]), u1 = crux_u32x2_to_f64(a.v[2], a.v[3]), u2 = crux_u32x2_to_f64(b.v[0], b.v[1]), u3 = crux_u32x2_to_f64(b.v[2], b.v[3]);
  if (kind == CRUX_ENV_CARTPOLE) { s[0] = __dadd_rn(-0.05, __dmul_rn(0.1, u0)); s[1] = __dadd_rn(-0.05, __dmul_rn(0.1, u1)); s[2] = __dadd_rn(-0.05, __dmul_rn(0.1, u2)); s[3] = __dadd_rn(-0.05, __dmul_rn(0.1, u3)); }
  else if (kind == CRUX_ENV_PENDULUM) { s[0] = __dadd_rn(-PI_D, __dmul_rn(2.0 * PI_D, u0)); s[1] = __dadd_rn(-1.0, __dmul_rn(2.0, u1)); }
  else { s[0] = 1.0 + floor(10.0 * u0); s[1] = 1.0 + floor(10.0 * u1); }
}
__device__ __forceinline__ float randn_f32(uint64_t seed, uint64_t ctr, uint32_t stream, int which) {
  const crux_u32x4 x = crux_philox(seed, ctr, stream, CRUX_RNG_NOISE);
  const double u1 = crux_u32x2_to_f64(x.v[0], x.v[1]), u2 = crux_u32x2_to_f64(x.v[2], x.v[3]);
  const double rr = sqrt(-2.0 * log(1.0 - u1)), th = 2.0 * PI_D * u2;
  return (float)(which ? rr * sin(th) : rr * cos(th));
}
__device__ __forceinline__ double linear_decay(double start, double stop, int64_t steps, int64_t i) {
  const double rate = (start - stop) / (double)steps; const double val = start - (double)i * rate; return val > stop ? val : stop;
}

struct RolloutArgs {
  NetDesc nd; const float* p;
  int32_t kind, E, max_steps, od, ad, sd, act_kind;
  uint64_t seed;
  const float* mu; const float* sigma;
  double* state; int64_t* ep_len; int64_t* n_resets; int64_t* steps_taken; float* svec; double* acc;
  float* S; void* A; float* SP; float* R; uint8_t* D; uint8_t* EE; float* LP; int64_t* TT; int64_t* II; float* W; float* RET; float* ADV;
  float* COST; float* CADV; float* CRET;      // :cost, :cost_advantage, :cost_return (cost-constrained solvers; NULL = absent)
  int64_t base, C, T;
  crux_rollout_cfg cfg;
  float squash;      // SquashedGaussianPolicy ascale, 0 = GaussianPolicy
  int32_t sigma_head;      // two-headed policy handle (crux_mlp_set_sigma_head): z holds 2 ad rows, [mu; logSigma]. Read by k_explore_generic only (the rollout side is dispatched by the host: k_rollout_sigma / k_rollout_wide_sigma). (Sits in what was padding: the struct keeps its size)
  // push!'s priority bookkeeping finished by the rollout launch itself (k_rollout_res with one environment; per_tree.h: push_touch_block); pt_pr == NULL: not asked for
  int64_t* pt_ids; float* pt_pr; float* pt_pminmax; float* pt_run; float* pt_total; float pt_alpha; int32_t pt_nlev, pt_touch; int64_t pt_N;
};

// exploration(pi_explore, svec; pi_on, i) / action(pi, svec) (sampler.jl:73; policies.jl:124-144, 338-344, 372-394, 466-494, 499-514) given the network outputs z of ONE
// observation: the action (aout: one-hot floats for the discrete heads, the action vector otherwise; ai: the discrete index) and its log-probability. Every draw is
// crux_philox(seed, f(ctr), stream = e, purpose) with ctr = the number of steps sampler e has taken so far -- shared by the rollout kernels (device environments) and
// k_policy_explore (caller-stepped environments, crux_policy_explore), so the two produce the same actions from the same observations.
__device__ __forceinline__ void rollout_head(const RolloutArgs& a, const float* z, const int ad, const int nout, const int e, const uint64_t gi, const uint64_t ctr,
                                             float* aout, int& ai, float& logprob) {
      logprob = NAN; ai = 0;
      if (a.cfg.head == CRUX_HEAD_CATEGORICAL || a.cfg.head == CRUX_HEAD_GREEDY_Q) {
        int greedy = 0; for (int q = 1; q < nout; ++q) if (z[q] > z[greedy]) greedy = q;
        if (!a.cfg.explore) ai = greedy;
        else if (a.cfg.eps_steps > 0 || a.cfg.head == CRUX_HEAD_GREEDY_Q) {
          const double eps = a.cfg.eps_steps > 0 ? linear_decay(a.cfg.eps_start, a.cfg.eps_stop, a.cfg.eps_steps, (int64_t)gi) : 0.0;
          const crux_u32x4 x = crux_philox(a.seed, ctr, (uint32_t)e, CRUX_RNG_ACTION);
          const double u = crux_u32x2_to_f64(x.v[0], x.v[1]);
          if (u < eps) { const crux_u32x4 y = crux_philox(a.seed, ctr, (uint32_t)e, CRUX_RNG_RANDACT); ai = (int)(((uint64_t)y.v[0] * (uint64_t)nout) >> 32); }
          else ai = greedy;
          if (a.LP) logprob = (float)log(eps * (1.0 / (double)nout) + (1.0 - eps));      // (a Float64 log per step: only where a :logprob column takes it)
        } else {
          float pr[ENV_MAXOBS];
          const float ldiv = a.cfg.logit_div > 0.f ? a.cfg.logit_div : 1.f;                       // softmax(value ./ alpha) (softq.jl:53)
          float mx = __fdiv_rn(z[0], ldiv); for (int q = 1; q < nout; ++q) { const float zq = __fdiv_rn(z[q], ldiv); mx = zq > mx ? zq : mx; }
          float sum = 0.f; for (int q = 0; q < nout; ++q) { pr[q] = expf(__fdiv_rn(z[q], ldiv) - mx); sum = __fadd_rn(sum, pr[q]); }
          for (int q = 0; q < nout; ++q) pr[q] = __fdiv_rn(pr[q], sum);
          const crux_u32x4 x = crux_philox(a.seed, ctr, (uint32_t)e, CRUX_RNG_ACTION);
          const float draw = crux_u32_to_f32(x.v[0]);
          float cp = pr[0]; ai = 0; while (cp <= draw && ai < nout - 1) { ai += 1; cp = __fadd_rn(cp, pr[ai]); }
          logprob = logf(pr[ai]);
        }
        for (int q = 0; q < ad; ++q) aout[q] = (q == ai) ? 1.f : 0.f;
      } else if (a.cfg.head == CRUX_HEAD_GAUSSIAN) {
        const float* ls = a.p + a.nd.xoff; float lp = 0.f;
        for (int q = 0; q < ad; ++q) {
          const float mu = z[q];
          if (a.squash > 0.f) {                                                   // SquashedGaussianPolicy (policies.jl:372, 388-394)
            if (a.cfg.explore) { const float sg = expf(sq_clampls(ls[q]));
              const float epsn = randn_f32(a.seed, ctr * (uint64_t)((ad + 1) / 2) + (uint64_t)(q / 2), (uint32_t)e, q & 1);
              const float u = __fadd_rn(__fmul_rn(epsn, sg), mu); const float s2 = __fmul_rn(sg, sg); const float dd = __fsub_rn(u, mu);
              aout[q] = __fmul_rn(a.squash, tanhf(u));
              lp = __fadd_rn(lp, __fsub_rn(__fsub_rn(__fsub_rn(__fdiv_rn(-__fmul_rn(dd, dd), __fmul_rn(2.f, s2)), 0.9189385332046727f), ls[q]), sq_corr(u))); }
            else aout[q] = __fmul_rn(a.squash, tanhf(mu));
          } else
          if (a.cfg.explore) { const float sg = expf(ls[q]);
            const float epsn = randn_f32(a.seed, ctr * (uint64_t)((ad + 1) / 2) + (uint64_t)(q / 2), (uint32_t)e, q & 1);
            aout[q] = __fadd_rn(__fmul_rn(epsn, sg), mu); const float s2 = __fmul_rn(sg, sg); const float dd = __fsub_rn(aout[q], mu);
            lp = __fadd_rn(lp, __fsub_rn(__fsub_rn(__fdiv_rn(-__fmul_rn(dd, dd), __fmul_rn(2.f, s2)), 0.9189385332046727f), ls[q])); }
          else aout[q] = mu;
        }
        logprob = a.cfg.explore ? lp : NAN;
      } else {
        for (int q = 0; q < ad; ++q) { float av = z[q];
          if (a.cfg.explore && a.cfg.noise_sigma >= 0.f) {
            float n0 = __fmul_rn(randn_f32(a.seed, ctr * (uint64_t)((ad + 1) / 2) + (uint64_t)(q / 2), (uint32_t)e, q & 1), a.cfg.noise_sigma);
            n0 = n0 < a.cfg.noise_eps_min ? a.cfg.noise_eps_min : n0 > a.cfg.noise_eps_max ? a.cfg.noise_eps_max : n0; av = __fadd_rn(av, n0);
            av = av < a.cfg.a_min ? a.cfg.a_min : av > a.cfg.a_max ? a.cfg.a_max : av; }
          aout[q] = av; }
      }
      if (a.cfg.explore == 2) logprob = NAN;      // action(pi, s) of an always_stochastic policy: exploration(pi, s)[1] with logprob NaN (policies.jl:124, sampler.jl:73)
}
// The head of a two-headed Gaussian policy handle (z = [mu; logSigma(s)], 2 ad rows; policies.jl:338-344, 372-394, 510-513), instantiated by the generic kernels only
// (k_rollout_sigma, k_rollout_wide_sigma -- k_rollout's and k_rollout_wide's body with this head --, k_explore_generic): the register-resident kernels never see such a handle and keep rollout_head's code as it was.
//   CRUX_HEAD_GAUSSIAN       exploration(pi, s): rollout_head's normals and operation order, logSigma read from z[ad + q]; squashed: its clamp and tanh correction
//   CRUX_HEAD_DETERMINISTIC  action(pi_on, s) = mu, ascale tanh(mu) when squashed (policies.jl:372), THEN the Gaussian noise and its clamps (:510-513)
__device__ __forceinline__ void rollout_head_sigma(const RolloutArgs& a, const float* z, const int ad, const int e, const uint64_t ctr, float* aout, int& ai, float& logprob) {
      logprob = NAN; ai = 0;
      if (a.cfg.head == CRUX_HEAD_GAUSSIAN) { float lp = 0.f;
        for (int q = 0; q < ad; ++q) { const float mu = z[q], ls = z[ad + q];
          if (!a.cfg.explore) { aout[q] = a.squash > 0.f ? __fmul_rn(a.squash, tanhf(mu)) : mu; continue; }
          const float sg = expf(a.squash > 0.f ? sq_clampls(ls) : ls);
          const float epsn = randn_f32(a.seed, ctr * (uint64_t)((ad + 1) / 2) + (uint64_t)(q / 2), (uint32_t)e, q & 1);
          const float u = __fadd_rn(__fmul_rn(epsn, sg), mu); const float s2 = __fmul_rn(sg, sg); const float dd = __fsub_rn(u, mu);
          float t = __fsub_rn(__fsub_rn(__fdiv_rn(-__fmul_rn(dd, dd), __fmul_rn(2.f, s2)), 0.9189385332046727f), ls);
          if (a.squash > 0.f) { t = __fsub_rn(t, sq_corr(u)); aout[q] = __fmul_rn(a.squash, tanhf(u)); } else aout[q] = u;
          lp = __fadd_rn(lp, t); }
        logprob = a.cfg.explore ? lp : NAN;
      } else {
        for (int q = 0; q < ad; ++q) { float av = a.squash > 0.f ? __fmul_rn(a.squash, tanhf(z[q])) : z[q];
          if (a.cfg.explore && a.cfg.noise_sigma >= 0.f) {
            float n0 = __fmul_rn(randn_f32(a.seed, ctr * (uint64_t)((ad + 1) / 2) + (uint64_t)(q / 2), (uint32_t)e, q & 1), a.cfg.noise_sigma);
            n0 = n0 < a.cfg.noise_eps_min ? a.cfg.noise_eps_min : n0 > a.cfg.noise_eps_max ? a.cfg.noise_eps_max : n0; av = __fadd_rn(av, n0);
            av = av < a.cfg.a_min ? a.cfg.a_min : av > a.cfg.a_max ? a.cfg.a_max : av; }
          aout[q] = av; }
      }
      if (a.cfg.explore == 2) logprob = NAN;
}
// Everything of step! after the policy forward (sampler.jl:73-136): action + logprob from the head, env transition, column writes,
// episode bookkeeping. `writer` lanes store to the buffer; all callers advance identical copies of the sampler state.
template <bool SIGMA = false>      // SIGMA: the two-headed head (generic kernels only)
__device__ __forceinline__ void rollout_tail(const RolloutArgs& a, const float* z, const int od, const int ad, const int nout, const int kind, const int e,
                                             const int64_t t, const int64_t j, const bool writer, double* st, int64_t& ep_len, int64_t& n_resets,
                                             int64_t& steps_taken, double& sum_r, int64_t& nee, float* next_obs, const int par_lane = -1,
                                             const float* mu_cached = nullptr, const float* sigma_cached = nullptr) {
  const float* mu = mu_cached ? mu_cached : a.mu; const float* sg = sigma_cached ? sigma_cached : a.sigma;      // (a kernel may hold the observation normalisation in LDS / registers)
  const int sd = kind == CRUX_ENV_CARTPOLE ? 4 : (env_is_synth(kind) ? od : 2);      // (SYNTH keeps one Float64 per observation: a compile-time od makes the state array registers)
      const uint64_t gi = a.cfg.i0 + (uint64_t)t * (uint64_t)a.E + (uint64_t)e;    // i + (j-1), env-minor (sampler.jl:161-163)
      const uint64_t ctr = (uint64_t)steps_taken;
      float logprob; int ai; float aout[ENV_MAXOBS];
      if constexpr (SIGMA) rollout_head_sigma(a, z, ad, e, ctr, aout, ai, logprob); else
      rollout_head(a, z, ad, nout, e, gi, ctr, aout, ai, logprob);
      // ---- env transition (sampler.jl:93-97)
      double sn[ENV_MAXSD]; float r; uint8_t done; float o[ENV_MAXOBS], spv[ENV_MAXOBS];
      if (kind == CRUX_ENV_CARTPOLE) cartpole_step(st, ai, sn, &r, &done);
      else if (kind == CRUX_ENV_PENDULUM) pendulum_step(st, aout[0], sn, &r, &done);
      else if (env_is_synth(kind)) synth_step(od, ad, kind == CRUX_ENV_SYNTH_DISCRETE, st, ai, aout, sn, &r, &done, par_lane);
      else { const crux_u32x4 xd = crux_philox(a.seed, ctr, (uint32_t)e, CRUX_RNG_ENVDYN); gridworld_step(st, ai, crux_u32x2_to_f64(xd.v[0], xd.v[1]), sn, &r, &done); }
      env_obs(kind, sn, o, od);
      for (int q = 0; q < od; ++q) spv[q] = __fdiv_rn(__fsub_rn(o[q], mu[q]), sg[q]);
      // ---- column writes (sampler.jl:101-107)
      if (writer) {
        if (a.act_kind == CRUX_ACTION_DISCRETE) { uint8_t* A = (uint8_t*)a.A + (size_t)j * ad; for (int q = 0; q < ad; ++q) A[q] = aout[q] != 0.f; }
        else { float* A = (float*)a.A + (size_t)j * ad; for (int q = 0; q < ad; ++q) A[q] = aout[q]; }
        for (int q = 0; q < od; ++q) a.SP[(size_t)j * od + q] = spv[q];
        a.R[j] = r; a.D[j] = done;
        if (a.LP) a.LP[j] = logprob;
        if (a.TT) a.TT[j] = ep_len + 1;
        if (a.II) a.II[j] = (int64_t)gi + 1;
        if (a.W) a.W[j] = 1.0f;
        if (a.RET) a.RET[j] = 0.f;
        if (a.ADV) a.ADV[j] = 0.f;
        if (a.COST) a.COST[j] = env_cost(kind, od, sn);                              // data[:cost][1,j] = info["cost"] (sampler.jl:114)
        if (a.CADV) a.CADV[j] = 0.f;
        if (a.CRET) a.CRET[j] = 0.f;
      }
      sum_r += (double)r; steps_taken += 1;
      // ---- episode bookkeeping (sampler.jl:130-136; terminate_episode! :53-69)
      ep_len += 1;
      uint8_t ee = 0;
      if (done || ep_len >= a.max_steps) {
        ee = 1; ++nee;
        env_draw_initial(kind, a.seed, (uint64_t)n_resets, (uint32_t)e, st, sd); n_resets += 1; ep_len = 0;
        env_obs(kind, st, o, od);
        for (int q = 0; q < od; ++q) next_obs[q] = __fdiv_rn(__fsub_rn(o[q], mu[q]), sg[q]);
      } else {
        for (int i = 0; i < sd; ++i) st[i] = sn[i];
        for (int q = 0; q < od; ++q) next_obs[q] = spv[q];
      }
      if (a.cfg.reset_at_end && t == a.T - 1 && ep_len > 0) {                       // sampler.jl:148
        ee = 1; ++nee;
        env_draw_initial(kind, a.seed, (uint64_t)n_resets, (uint32_t)e, st, sd); n_resets += 1; ep_len = 0;
        env_obs(kind, st, o, od);
        for (int q = 0; q < od; ++q) next_obs[q] = __fdiv_rn(__fsub_rn(o[q], mu[q]), sg[q]);
      }
      if (writer) a.EE[j] = ee;
}

template <int CTRL> __device__ __forceinline__ float env_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float env_wave_sum_uniform(float v) {      // the same bits in every lane (readfirstlane of one reduction order)
  v += env_dpp<0x128>(v); v += env_dpp<0x124>(v); v += env_dpp<0x122>(v); v += env_dpp<0x121>(v);     // row_ror 8,4,2,1: row totals
  float a0 = v, b0 = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a0), "+v"(b0));
  a0 = a0 + b0; b0 = a0;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a0), "+v"(b0));
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a0 + b0)));
}
// the forward pass of the register-resident IN-64-64-OUT policy on ONE observation, by one wave: lane j holds row j of W1 / W2 and column j of W3. Layers 1 and 2 are fma chains over
// k ascending (+ bias, activation), layer 3 a product per lane summed over the wave in one fixed order. Shared by k_rollout_h64 and k_explore_h64 (same bits from the same observation).
template <int IN, int OUT, int ACT>
__device__ __forceinline__ void h64_forward(const float (&w1)[IN], const float (&w2)[64], const float (&w3)[OUT], const float (&b3)[OUT], const float b1, const float b2,
                                            const float (&x)[IN], float* sh, const int lane, float (&z)[OUT]) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < IN; ++k) acc = fmaf(w1[k], x[k], acc);
    sh[lane] = crux_act(ACT, acc + b1);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    acc = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < 16; ++k4) { const float4 hv = *(const float4*)&sh[4 * k4];
      acc = fmaf(w2[4 * k4], hv.x, acc); acc = fmaf(w2[4 * k4 + 1], hv.y, acc); acc = fmaf(w2[4 * k4 + 2], hv.z, acc); acc = fmaf(w2[4 * k4 + 3], hv.w, acc); }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    const float h2 = crux_act(ACT, acc + b2);
#pragma unroll
    for (int o = 0; o < OUT; ++o) z[o] = env_wave_sum_uniform(w3[o] * h2) + b3[o];
}
// one wave (64 lanes) per environment; lanes split the output units of each Dense layer, lane 0 runs the
// head, the dynamics and the bookkeeping. Environments never synchronise with each other.
// The body is a device function of ONE wave (its LDS traffic is ordered by a wave barrier, not a workgroup barrier), so that the small-network
// solve kernel (small_solve.hip) can run it on one of its waves.
#define RO_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
// NT = threads sharing the body: 64 (one wave, ordered by a wave barrier) or 256 (one workgroup per environment, ordered by __syncthreads: the wide-network rollout
// kernel k_rollout_wide -- with 256-wide layers one wave needed 117 us per step). Thread 0 runs the tail either way; the layer arithmetic (fma over k ascending, + bias,
// activation) is the same, so the results are.
// Chain(Dense...) on ONE observation held in hbuf[0] (sampler.jl:73 -> policies.jl:94,120) by NT threads: thread o evaluates output unit o (fma over k ascending, + bias,
// activation); returns the index of the hbuf half that holds the outputs. Shared by the generic rollout kernels and k_explore_generic.
template <int NT>
__device__ __forceinline__ int rollout_generic_forward(const RolloutArgs& a, const int lane, float (*hbuf)[1024]) {
    const NetDesc& nd = a.nd;
    int cur = 0;
    for (int l = 0; l < nd.L; ++l) {
      const int in = nd.dims[l], out = nd.dims[l + 1], act = nd.acts[l];
      const float* Wl = a.p + nd.woff[l]; const float* bl = a.p + nd.boff[l];
      for (int o = lane; o < out; o += NT) {
        float accv = 0.f; int k = 0;
        if (NT > 64) {                         // wide layers (one workgroup per environment): 32 independent weight loads in flight -- a batch-1 layer is a chain of L2 round trips,
          for (; k + 32 <= in; k += 32) {      // and its length is in / (loads in flight); the fma chain keeps its order, so the result keeps its bits
            float wv[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) wv[u] = Wl[o + out * (k + u)];
#pragma unroll
            for (int u = 0; u < 32; ++u) accv = fmaf(wv[u], hbuf[cur][k + u], accv); } }
        for (; k + 8 <= in; k += 8) {          // eight independent weight loads in flight; the fma chain keeps its order
          float wv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) wv[u] = Wl[o + out * (k + u)];
#pragma unroll
          for (int u = 0; u < 8; ++u) accv = fmaf(wv[u], hbuf[cur][k + u], accv); }
        for (; k < in; ++k) accv = fmaf(Wl[o + out * k], hbuf[cur][k], accv);
        hbuf[cur ^ 1][o] = crux_act(act, accv + bl[o]);
      }
      if (NT == 64) { RO_WAVE_SYNC(); } else { __syncthreads(); }
      cur ^= 1;
    }
    return cur;
}
template <int NT = 64, bool HEADS2 = false>      // HEADS2: the instantiations for two-headed policy handles (k_rollout_sigma, k_rollout_wide_sigma); every other one is as it was
__device__ __forceinline__ void rollout_generic_wave(const RolloutArgs& a, const int e, const int lane, float (*hbuf)[1024], float* sh_misc) {
#define RO_SYNC() do { if (NT == 64) { RO_WAVE_SYNC(); } else { __syncthreads(); } } while (0)
  const NetDesc& nd = a.nd;
  const int od = a.od, ad = a.ad, nout = nd.dims[nd.L];
  double st[ENV_MAXSD]; int64_t ep_len = 0, n_resets = 0, steps_taken = 0; double sum_r = 0.0; int64_t nee = 0;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < ENV_MAXSD; ++i) if (i < a.sd) st[i] = a.state[(size_t)e * a.sd + i];      // constant indices: the state array stays in registers
    ep_len = a.ep_len[e]; n_resets = a.n_resets[e]; steps_taken = a.steps_taken[e];
  }
  if (lane < od) hbuf[0][lane] = a.svec[(size_t)e * od + lane];
  RO_SYNC();
  for (int64_t t = 0; t < a.T; ++t) {
    const int64_t j = (a.base + (int64_t)e * a.T + t) % a.C;
    // current observation -> S column (sampler.jl:100)
    if (lane < od) a.S[(size_t)j * od + lane] = hbuf[0][lane];
    // ---- policy forward: Chain(Dense...) on a batch of one (sampler.jl:73 -> policies.jl:94,120)
    const int cur = rollout_generic_forward<NT>(a, lane, hbuf);
    // (the observation in hbuf[0] was already stored to the S column, so the ping-pong may overwrite it)
    // the tail with compile-time kind and dimensions for the restated environments (its per-step arrays are then registers; with run-time dimensions they are
    // private memory and the step costs ~3x more), the run-time form for everything else (SYNTH envs of any width)
    if (lane == 0) {
      if constexpr (HEADS2) {      // (nout = 2 ad here; Pendulum, the SAC examples' environment, gets its compile-time tail as below)
        if (a.kind == CRUX_ENV_PENDULUM && od == 3 && ad == 1 && nout == 2) rollout_tail<true>(a, hbuf[cur], 3, 1, 2, CRUX_ENV_PENDULUM, e, t, j, true, st, ep_len, n_resets, steps_taken, sum_r, nee, sh_misc);
        else rollout_tail<true>(a, hbuf[cur], od, ad, nout, a.kind, e, t, j, true, st, ep_len, n_resets, steps_taken, sum_r, nee, sh_misc);
      } else
      if (a.kind == CRUX_ENV_CARTPOLE && od == 4 && ad == 2 && nout == 2) rollout_tail(a, hbuf[cur], 4, 2, 2, CRUX_ENV_CARTPOLE, e, t, j, true, st, ep_len, n_resets, steps_taken, sum_r, nee, sh_misc);
      else if (a.kind == CRUX_ENV_GRIDWORLD && od == 2 && ad == 4 && nout == 4) rollout_tail(a, hbuf[cur], 2, 4, 4, CRUX_ENV_GRIDWORLD, e, t, j, true, st, ep_len, n_resets, steps_taken, sum_r, nee, sh_misc);
      else if (a.kind == CRUX_ENV_PENDULUM && od == 3 && ad == 1 && nout == 1) rollout_tail(a, hbuf[cur], 3, 1, 1, CRUX_ENV_PENDULUM, e, t, j, true, st, ep_len, n_resets, steps_taken, sum_r, nee, sh_misc);
      else if (a.kind == CRUX_ENV_SYNTH_DISCRETE && od == 8 && ad == 4 && nout == 4) rollout_tail(a, hbuf[cur], 8, 4, 4, CRUX_ENV_SYNTH_DISCRETE, e, t, j, true, st, ep_len, n_resets, steps_taken, sum_r, nee, sh_misc);
      else rollout_tail(a, hbuf[cur], od, ad, nout, a.kind, e, t, j, true, st, ep_len, n_resets, steps_taken, sum_r, nee, sh_misc);
    }
    RO_SYNC();
    if (lane < od) hbuf[0][lane] = sh_misc[lane];
    RO_SYNC();
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < ENV_MAXSD; ++i) if (i < a.sd) a.state[(size_t)e * a.sd + i] = st[i];
    a.ep_len[e] = ep_len; a.n_resets[e] = n_resets; a.steps_taken[e] = steps_taken;
    a.acc[2 * e] = sum_r; a.acc[2 * e + 1] = (double)nee;
  }
  if (lane < od) a.svec[(size_t)e * od + lane] = hbuf[0][lane];
}
static void fill_rollout_args(RolloutArgs& a, crux_env* e, crux_mlp* policy, const crux_rollout_cfg* cfg, crux_buffer* buf, int64_t T) {
  a = RolloutArgs{};
  a.nd = policy->nd; a.p = policy->p; a.kind = e->kind; a.E = e->n_envs; a.max_steps = e->max_steps; a.od = e->obs_dim; a.ad = e->act_dim; a.sd = e->state_dim;
  a.act_kind = buf->act_kind; a.seed = e->seed; a.mu = e->mu; a.sigma = e->sigma; a.state = e->state; a.ep_len = e->ep_len; a.n_resets = e->n_resets;
  a.steps_taken = e->steps_taken; a.svec = e->svec; a.acc = e->acc;
  a.S = (float*)buf->col[CRUX_COL_S]; a.A = buf->col[CRUX_COL_A]; a.SP = (float*)buf->col[CRUX_COL_SP]; a.R = (float*)buf->col[CRUX_COL_R];
  a.D = (uint8_t*)buf->col[CRUX_COL_DONE]; a.EE = (uint8_t*)buf->col[CRUX_COL_EPISODE_END];
  a.LP = has_col(buf, CRUX_COL_LOGPROB) ? (float*)buf->col[CRUX_COL_LOGPROB] : nullptr; a.TT = has_col(buf, CRUX_COL_T) ? (int64_t*)buf->col[CRUX_COL_T] : nullptr;
  a.II = has_col(buf, CRUX_COL_I) ? (int64_t*)buf->col[CRUX_COL_I] : nullptr; a.W = has_col(buf, CRUX_COL_WEIGHT) ? (float*)buf->col[CRUX_COL_WEIGHT] : nullptr;
  a.RET = has_col(buf, CRUX_COL_RETURN) ? (float*)buf->col[CRUX_COL_RETURN] : nullptr; a.ADV = has_col(buf, CRUX_COL_ADVANTAGE) ? (float*)buf->col[CRUX_COL_ADVANTAGE] : nullptr;
  a.COST = has_col(buf, CRUX_COL_COST) ? (float*)buf->col[CRUX_COL_COST] : nullptr; a.CADV = has_col(buf, CRUX_COL_COST_ADVANTAGE) ? (float*)buf->col[CRUX_COL_COST_ADVANTAGE] : nullptr;
  a.CRET = has_col(buf, CRUX_COL_COST_RETURN) ? (float*)buf->col[CRUX_COL_COST_RETURN] : nullptr;
  a.base = buf->next_ind; a.C = buf->capacity; a.T = T; a.cfg = *cfg; a.squash = policy->squash; a.sigma_head = policy->sigma_head ? 1 : 0;
}
// the (sum of rewards, episode ends) pairs the rollout kernels leave per environment in acc [2 x E] (a host copy) -> the totals steps! reports; either output may be NULL
static void rollout_acc_sum(const double* acc, int E, double* sum_r, int64_t* n_episode_end) {
  double sr = 0; int64_t ne = 0; for (int k = 0; k < E; ++k) { sr += acc[2 * k]; ne += (int64_t)acc[2 * k + 1]; }
  if (sum_r) *sum_r = sr; if (n_episode_end) *n_episode_end = ne; }
static bool is_h64(const NetDesc& nd) { return nd.L == 3 && nd.dims[1] == 64 && nd.dims[2] == 64 && nd.acts[0] == nd.acts[1] && nd.acts[2] == CRUX_ACT_IDENTITY; }      // h64_forward's family
// THE list of instantiated (IN, OUT, ACT, KIND) shapes of k_rollout_h64 / k_explore_h64 (env.hip): the rollout, the batched rollout and the explore dispatch expand it, so a
// row added here serves all three -- crux_policy_explore promises the bits of the rollout kernel that serves the policy shape. Explore ignores KIND: the triples are distinct.
#define H64_SHAPES(X) \
  X(4, 2, CRUX_ACT_RELU, CRUX_ENV_CARTPOLE) X(4, 2, CRUX_ACT_TANH, CRUX_ENV_CARTPOLE) \
  X(3, 1, CRUX_ACT_RELU, CRUX_ENV_PENDULUM) X(3, 1, CRUX_ACT_TANH, CRUX_ENV_PENDULUM) \
  X(17, 6, CRUX_ACT_TANH, CRUX_ENV_SYNTH)   X(17, 6, CRUX_ACT_RELU, CRUX_ENV_SYNTH)       /* C5-shaped: 17 obs / 6 continuous actions */
