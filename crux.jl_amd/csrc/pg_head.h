// pg_head.h -- one sample of ppo_loss / a2c_loss (rl/ppo.jl:4-21, a2c.jl:4-15) under a categorical head (policies.jl:135,152-155), written once for the dense-engine learner's
// head (k_pg_head, train_dense.hip), the conv learner's column head (k_conv_pg_head, conv_pair.hip) and the conv BC head (k_conv_bc_head, conv_bc.hip). All live in the translation unit that is compiled without contraction,
// so the callers form the same bits.
#pragma once
#include "mfma_helpers.h"      // EPS32F

// what the caller adds to its Float64 statistics: the surrogate term (newlp * A for a2c_loss), the entropy, log pi(a|s), the ratio (1 for a2c_loss) and lagrange_ppo_loss's cost term
struct PgCatTerms { float lossp, H, newlp, r, cost; };
// z, dy: the sample's nout logits and their seed d(loss)/dz (already divided by the batch: invB); av: its one-hot action. lagr: lagrange_ppo_loss (ppo.jl:70-131) with the
// penalty `pen` and the cost advantage Ac. SEED = false (the forward-only loss pass of conv_bc.hip): the terms alone, dy is not touched.
template <bool SEED = true>
__device__ __forceinline__ PgCatTerms pg_categorical_sample(const float* __restrict__ z, const int nout, const uint8_t* __restrict__ av, const float A, const float oldlp, const float lo, const float hi,
                                                            const float lambda_p, const float lambda_e, const bool a2c, const float invB, const bool lagr, const float pen, const float Ac, float* __restrict__ dy) {
  PgCatTerms o; float H = 0.f, r, g;
  float mx = z[0]; for (int k = 1; k < nout; ++k) mx = z[k] > mx ? z[k] : mx;
  float sum = 0.f; for (int k = 0; k < nout; ++k) sum += expf(z[k] - mx);
  float qq = 0.f, hp = 0.f;
  for (int k = 0; k < nout; ++k) { const float pk = expf(z[k] - mx) / sum; qq += pk * (av[k] ? 1.f : 0.f);
    const float lg = logf(pk + EPS32F); H -= pk * lg; hp += (-lg - pk / (pk + EPS32F)) * pk; }
  const float newlp = logf(qq);
  r = expf(newlp - oldlp); const float u = r * A, rc = fminf(fmaxf(r, lo), hi), cl = rc * A;
  g = (u <= cl) ? A : 0.f; o.lossp = a2c ? newlp * A : (u <= cl ? u : cl);
  if (a2c) { g = A; r = 1.f; }
  float gcr = 0.f; o.cost = 0.f;
  if (lagr) { const float uc = r * Ac, clc = rc * Ac; o.cost = uc >= clc ? uc : clc; gcr = (uc >= clc ? Ac : 0.f) * r; }
  if (SEED) for (int k = 0; k < nout; ++k) { const float pk = expf(z[k] - mx) / sum; const float lg = logf(pk + EPS32F); const float hk = -lg - pk / (pk + EPS32F);
    const float dlogpi = pk * ((av[k] ? 1.f : 0.f) / qq) - pk;
    const float base = -lambda_p * g * r * dlogpi - lambda_e * (pk * (hk - hp));
    dy[k] = lagr ? invB * ((base + pen * gcr * dlogpi) / (1.f + pen)) : invB * base; }
  o.H = H; o.newlp = newlp; o.r = r; return o;
}

// One sample of a GaussianPolicy with a constant logSigma (policies.jl:333-348): log pi(a|s) = sum_d [-(a_d - mu_d)^2 / (2 sigma_d^2) - log(2 pi) / 2 - logSigma_d] in the
// operation order of k_pg_head's Gaussian branch (train_dense.hip), and slot d's pair of derivatives under the weight cf = d(loss)/d(log pi): the seed
// d(loss)/d(mu_d) = (1/B) cf (a_d - mu_d) / sigma_d^2 and the sample's share of d(loss)/d(logSigma_d) = (1/B) cf ((a_d - mu_d)^2 / sigma_d^2 - 1).
__device__ __forceinline__ float pg_gauss_logpdf(const float* __restrict__ mu, const float* __restrict__ av, const float* __restrict__ ls, const int ad) {
  float lp = 0.f;
  for (int k = 0; k < ad; ++k) { const float lk = ls[k]; const float sg = expf(lk); const float d = av[k] - mu[k];
    lp += (-(d * d) / (2.f * sg * sg) - 0.9189385332046727f - lk); }
  return lp;
}
struct PgGaussSlot { float dmu, dls; };
__device__ __forceinline__ PgGaussSlot pg_gauss_slot(const float mu, const float a, const float lk, const float cf, const float invB) {
  const float sg = expf(lk); const float s2 = sg * sg; const float d = a - mu;
  return PgGaussSlot{invB * (cf * (d / s2)), invB * (cf * ((d * d) / s2 - 1.f))};
}
