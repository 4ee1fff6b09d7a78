// learner_shared.h -- what the two register-resident on-policy learner kernels, k_train_mfma (train_mfma_kernel.h) and k_train_fs2 (train_fs2_kernel.h), compute alike,
// written once. Everything here is a __device__ __forceinline__ function of VALUES (indices in, index out; pointers by value) with no floating-point arithmetic and no
// contraction pragma, so each definition compiles, in every translation unit that includes it, to the machine code of the inline copy it replaces
// (profiles/learner_shared_resources.txt has the per-kernel comparison, and what did not meet that bar and therefore stays written out at its call sites).
#pragma once
#include "train_args.h"
#include "mfma_helpers.h"

// ---- flat index spaces of the small parameters (everything but W2), from the layout type Lt (MfLayout / Fs2Layout) ---------------------------------------------------
// s = thread-owned index -> LDS master word / canonical (Flux.params) index / word inside a tile's partial block.
// H2 = width of the second hidden layer (its W3 rows), LD = row stride of the partial block's W1 rows.
template <class Lt, int OUT, int H2>
__device__ __forceinline__ int slot_master(int s) {
  if (s < Lt::sB1) { const int o = s & 63, i = s >> 6; return Lt::oW1R + o * Lt::W1LD + i; }
  if (s < Lt::sB2) return Lt::oB1 + (s - Lt::sB1);
  if (s < Lt::sW3) return Lt::oB2 + (s - Lt::sB2);
  if (s < Lt::sB3) { const int t = s - Lt::sW3; const int o = t % OUT, i = t / OUT; return Lt::oW3R + o * H2 + i; }
  if (s < Lt::sEX) return Lt::oB3 + (s - Lt::sB3);
  return Lt::oEX + (s - Lt::sEX);
}
template <class Lt>
__device__ __forceinline__ int slot_canon(int s) {
  if (s < Lt::sB1) return Lt::cW1 + s;
  if (s < Lt::sB2) return Lt::cB1 + (s - Lt::sB1);
  if (s < Lt::sW3) return Lt::cB2 + (s - Lt::sB2);
  if (s < Lt::sB3) return Lt::cW3 + (s - Lt::sW3);
  if (s < Lt::sEX) return Lt::cB3 + (s - Lt::sB3);
  return Lt::cEX + (s - Lt::sEX);
}
template <class Lt, int OUT, int H2, int LD>
__device__ __forceinline__ int slot_part(int s) {
  if (s < Lt::sB1) { const int o = s & 63, i = s >> 6; return Lt::pW1 + i * LD + o; }
  if (s < Lt::sB2) return Lt::pB1 + (s - Lt::sB1);
  if (s < Lt::sW3) return Lt::pB2 + (s - Lt::sB2);
  if (s < Lt::sB3) { const int t = s - Lt::sW3; const int o = t % OUT, i = t / OUT; return Lt::pW3 + o * H2 + i; }
  if (s < Lt::sEX) return Lt::pB3 + (s - Lt::sB3);
  return Lt::pEX + (s - Lt::sEX);
}

// ---- an epoch's row of epoch_infos ---------------------------------------------------------------------------------------------------------------------------------
// from the reported minibatch's info that thread 0 keeps in the LDS words Lt::iLOSS .. Lt::iPLOSS: aggregate_info(minibatch_infos) == the last minibatch.
// The KL is the caller's register (every thread's loop exit reads it).
template <class Lt, int KIND, bool LAG>
__device__ __forceinline__ void epoch_info_row(float* e, const float* sm, const float inf_kl) {
  for (int k = 0; k < CRUX_INFO_N; ++k) e[k] = 0.f;
  e[CRUX_INFO_LOSS] = sm[Lt::iLOSS]; e[CRUX_INFO_GRAD_NORM] = sm[Lt::iGN];
  if (KIND != MFK_VALUE) { e[CRUX_INFO_ENTROPY] = sm[Lt::iENT]; e[CRUX_INFO_KL] = inf_kl; e[CRUX_INFO_CLIP_FRACTION] = sm[Lt::iCLIP]; e[CRUX_INFO_AVG_ADVANTAGE] = sm[Lt::iADV]; e[CRUX_INFO_AVG_RETURN] = sm[Lt::iRET]; }
  if constexpr (LAG) { e[CRUX_INFO_PENALTY] = sm[Lt::iPEN]; e[CRUX_INFO_CUR_COST] = sm[Lt::iCUR]; e[CRUX_INFO_COST_LOSS] = sm[Lt::iCLOSS]; e[CRUX_INFO_P_LOSS] = sm[Lt::iPLOSS]; }
}
