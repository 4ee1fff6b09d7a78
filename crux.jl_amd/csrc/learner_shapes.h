// learner_shapes.h -- the ONE table of the register-resident on-policy learners: every shape of the IN -> 64 -> {64, 32} -> OUT family a kernel is instantiated for, and in
// which forms. The dispatchers (train_fs2.hip, train_mfma_x2.hip, train_mfma8.hip) instantiate from it, the route (learner_route.h) reads the same rows at run time, and
// tests/test_learner_cases.py reads this file. The forms: k_train_fs2 (train_fs2_kernel.h), the feature-split kernel on four compute units of one XCD -- full batch_train!
// loops with minibatches of 65..128 rows, its lagrange_ppo_loss (LAG) and replica-group (PX / PXK) instantiations, the only form with a 32-wide second layer and a second
// activation of its own -- and ONE kernel template (train_mfma_kernel.h: k_train_mfma<IN, OUT, KIND, ACT, NW, NWG, ...>) in two forms: exact-f32 v_mfma_f32_16x16x4_f32
// GEMMs for the 64-wide layers, the last layer and the loss head on the VALU, the 64x64 weight gradient model-parallel over waves with theta / m / v of W2 living in the
// owning wave's registers for the whole launch.
//   * <NW = 4, NWG = 2> (train_mfma_x2.hip): one learner on TWO compute units of an XCD; minibatches of 65..128 rows, and -- for the shapes the one-CU form does not
//     instantiate -- also single steps, gradient-only calls and small minibatches. Neither form exchanges gradients with a replica group.
//   * <NW = 8, NWG = 1> (train_mfma8.hip): one learner on ONE compute unit with 8 waves; narrow inputs (IN <= 4), any minibatch up to 128 rows, single steps (train!,
//     crux_loss_grad), and the population launches where compute units are the scarce resource.
#pragma once
#include "train_args.h"

enum { MFK_CATEGORICAL = 0, MFK_GAUSSIAN = 1, MFK_VALUE = 2 };
// (loss, head) -> MFK_*, -1 = no kernel head for it. Which losses a form accepts is the route's filter.
static inline int mf_kind(int loss, int head) {
  if (loss == CRUX_LOSS_VALUE_MSE) return MFK_VALUE;
  return head == CRUX_HEAD_CATEGORICAL ? MFK_CATEGORICAL : head == CRUX_HEAD_GAUSSIAN ? MFK_GAUSSIAN : -1;
}

// FORMS: one bit per form a row is instantiated in. k_train_fs2: LF_FS2 = its plain, PX and PXK instantiations (every row), _MIN = also in the -DCRUX_FS2_MINIMAL build (the four
// bench learners), _LAG = with the lagrange_ppo_loss controller (ppo.jl:70-131), _TIMING = with the phase timers (CRUX_MFMA_TIMING). k_train_mfma<..., 4, 2>: LF_X2, _LAG =
// dispatched with lagrange_ppo_loss (the LAG kernel itself is compiled for every policy row of LF_X2), _MULTI = in the population launch (crux_policy_gradient_training_multi),
// _TIMING. k_train_mfma<..., 8, 1>: LF_ONE8, _MULTI, _TIMING.
enum : unsigned { LF_FS2 = 1, LF_FS2_MIN = 2, LF_FS2_LAG = 4, LF_FS2_TIMING = 8, LF_X2 = 16, LF_X2_LAG = 32, LF_X2_MULTI = 64, LF_X2_TIMING = 128, LF_ONE8 = 256, LF_ONE8_MULTI = 512, LF_ONE8_TIMING = 1024 };
#ifdef CRUX_FS2_MINIMAL
constexpr unsigned LF_FS2_BUILT = LF_FS2_MIN;
#else
constexpr unsigned LF_FS2_BUILT = LF_FS2;
#endif
// X(IN, OUT, KIND, ACT, H2, ACT2, FORMS). The ORDER is data: tests/learner_cases.py derives the (bs, r) schedule of a row from its index.
#define CRUX_LEARNER_SHAPES(X) \
  X(4, 2, MFK_CATEGORICAL, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2 | LF_FS2_MIN | LF_FS2_LAG | LF_FS2_TIMING | LF_X2 | LF_X2_LAG | LF_X2_MULTI | LF_X2_TIMING | LF_ONE8 | LF_ONE8_MULTI | LF_ONE8_TIMING)   /* C2 actor (PPO CartPole) */ \
  X(4, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2 | LF_FS2_MIN | LF_FS2_TIMING | LF_X2 | LF_X2_MULTI | LF_ONE8 | LF_ONE8_MULTI)   /* C2 critic */ \
  X(17, 6, MFK_GAUSSIAN, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2 | LF_FS2_MIN | LF_FS2_LAG | LF_FS2_TIMING | LF_X2 | LF_X2_LAG | LF_X2_MULTI | LF_X2_TIMING)   /* C5 actor (PPO HalfCheetah-shaped, 17 obs / 6 act): 4 waves per workgroup keep the 17-wide layout of the two-CU form inside 160 KB */ \
  X(17, 1, MFK_VALUE, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2 | LF_FS2_MIN | LF_FS2_TIMING | LF_X2 | LF_X2_MULTI)   /* C5 critic */ \
  X(3, 1, MFK_GAUSSIAN, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2 | LF_X2 | LF_FS2_LAG | LF_X2_LAG | LF_ONE8 | LF_ONE8_MULTI)   /* Pendulum actor */ \
  X(3, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2 | LF_X2 | LF_ONE8 | LF_ONE8_MULTI)   /* Pendulum critic */ \
  X(17, 6, MFK_GAUSSIAN, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2 | LF_X2) \
  X(17, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2 | LF_X2) \
  X(8, 4, MFK_CATEGORICAL, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2 | LF_X2 | LF_FS2_LAG | LF_X2_LAG)   /* 8 observations / 4 discrete actions (LunarLander-shaped, the C3 environment under an on-policy learner) */ \
  X(8, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2 | LF_X2) \
  X(2, 1, MFK_GAUSSIAN, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2)   /* the reference's own Pendulum examples observe (theta, theta_dot): 2 inputs (examples/rl/pendulum.jl) */ \
  X(2, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(6, 3, MFK_CATEGORICAL, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2)   /* from here: standard Gym shapes -- Acrobot 6 / 3, MountainCar 2 / 3, LunarLanderContinuous 8 / 2, Hopper 11 / 3, BipedalWalker 24 / 4, Ant 27 / 8 */ \
  X(6, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(2, 3, MFK_CATEGORICAL, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(8, 2, MFK_GAUSSIAN, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(8, 2, MFK_GAUSSIAN, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2) \
  X(8, 1, MFK_VALUE, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2) \
  X(11, 3, MFK_GAUSSIAN, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(11, 3, MFK_GAUSSIAN, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2) \
  X(11, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(11, 1, MFK_VALUE, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2) \
  X(24, 4, MFK_GAUSSIAN, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2)   /* (where the W2 backups of the PX / PXK forms fit into LDS beside the kernel's own 113..132 KB they live there; the 24- and 27-input shapes keep them in registers: their periodic forms spill 2..61 registers, the per-step forms 0..4) */ \
  X(24, 4, MFK_GAUSSIAN, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2) \
  X(24, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(24, 1, MFK_VALUE, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2) \
  X(27, 8, MFK_GAUSSIAN, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(27, 8, MFK_GAUSSIAN, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2) \
  X(27, 1, MFK_VALUE, CRUX_ACT_RELU, 64, CRUX_ACT_RELU, LF_FS2) \
  X(27, 1, MFK_VALUE, CRUX_ACT_TANH, 64, CRUX_ACT_TANH, LF_FS2) \
  X(17, 6, MFK_GAUSSIAN, CRUX_ACT_TANH, 32, CRUX_ACT_TANH, LF_FS2)   /* the reference's HalfCheetah PPO networks (examples/rl/half_cheetah_mujoco.jl:33-38): mu = 17 -tanh-> 64 -tanh-> 32 -> 6, V = 17 -tanh-> 64 -> 32 -> 1 */ \
  X(17, 1, MFK_VALUE, CRUX_ACT_TANH, 32, CRUX_ACT_IDENTITY, LF_FS2) \
  X(17, 1, MFK_VALUE, CRUX_ACT_TANH, 32, CRUX_ACT_TANH, LF_FS2)

struct LearnerShape {      // the run-time view of a row
  int in, out, kind, act, h2, act2; unsigned forms;
  constexpr bool is(int i, int o, int k, int a, int h, int a2) const { return in == i && out == o && kind == k && act == a && h2 == h && act2 == a2; }
};
#define LEARNER_SHAPE_ROW_(I, O, K, A, H, A2, F) {I, O, K, A, H, A2, (F)},
inline constexpr LearnerShape LEARNER_SHAPES[] = {CRUX_LEARNER_SHAPES(LEARNER_SHAPE_ROW_)};
#undef LEARNER_SHAPE_ROW_
// every row is a k_train_fs2 row; the one- and two-CU forms take ONE activation for both hidden layers and a 64-wide second layer, the minimal build's rows have timers
#define LEARNER_SHAPE_CHECK_(I, O, K, A, H, A2, F) \
  static_assert(((F) & LF_FS2) && (!((F) & (LF_X2 | LF_ONE8 | LF_FS2_LAG | LF_FS2_TIMING)) || (H == 64 && A2 == A)) && (!((F) & (LF_FS2_LAG | LF_X2_LAG)) || K != MFK_VALUE), "learner row " #I "-" #O); \
  static_assert((!((F) & (LF_X2_LAG | LF_X2_MULTI | LF_X2_TIMING)) || ((F) & LF_X2)) && (!((F) & (LF_ONE8_MULTI | LF_ONE8_TIMING)) || ((F) & LF_ONE8)), "learner row " #I "-" #O);
CRUX_LEARNER_SHAPES(LEARNER_SHAPE_CHECK_)
#undef LEARNER_SHAPE_CHECK_
// the row of a network under a head (mf_kind), NULL outside the family -- IN -> 64 -> H2 -> OUT with an identity output layer -- or the table. A row with H2 != 64 or
// ACT2 != ACT carries the k_train_fs2 flags only.
static inline const LearnerShape* learner_shape(const NetDesc& nd, int kind) {
  if (nd.L != 3 || nd.dims[1] != 64 || nd.acts[2] != CRUX_ACT_IDENTITY || kind < 0) return nullptr;
  for (const LearnerShape& r : LEARNER_SHAPES) if (r.is(nd.dims[0], nd.dims[3], kind, nd.acts[0], nd.dims[2], nd.acts[1])) return &r;
  return nullptr;
}
