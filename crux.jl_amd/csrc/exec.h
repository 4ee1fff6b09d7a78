// exec.h -- the fused-step executor: a recorded sequence of kernel bodies run as a few launches, one per PHASE.
//
// The off-policy learners on wide networks (value_training, src/model_free/off_policy.jl:66-111: rand! -> target -> td_error / update_priorities! ->
// train!(critic) -> train!(actor) -> target update) are chains of 20-70 small dependent kernels; launched one by one each costs ~5 us whatever its
// size, so an epoch was launch-bound. In record mode the launch sites push an ExecOp {kernel body id, block count, packed arguments}
// instead of launching. The caller tags every op with a phase (ops of one phase do not depend on each other); crux_exec_run then launches each phase
// once over the whole chip: k_phase_k with the phase's records in the kernel arguments, or k_phase with them in a device copy of the list when they
// do not fit (exec.hip). The kernel boundary is the dependency between phases.
// The bodies are the SAME device functions the stand-alone kernels call (struct XOp::run), so both forms compute identical results.
//
// Adding an op takes two things:
//   1. `struct XOp { static __device__ __forceinline__ void run(const unsigned bid, const unsigned nblocks, args...); };` -- the body, written for block bid of nblocks
//      (plus `static constexpr int max_threads = N;` when its stand-alone kernel wants __launch_bounds__(N));
//   2. one line `X(OP_X, XOp, tail)` at the END of CRUX_EXEC_OPS below (the ids are positions in the list).
// Everything else follows from the type: the id (OpKid<XOp>), the argument pack (OpPack<XOp>), the case of the phase kernels' switch, the stand-alone kernel
// (k_op<XOp, ...>), and the launch sites -- CRUX_RUN(c, XOp, nblocks, NT, stream, args...) records or launches, crux_exec_push<XOp>(c, nblocks, args...) records,
// crux_launch<XOp>(nblocks, NT, stream, args...) launches and never records. A table line without a struct, or a recorded type without a table line, does not compile.
// An op body that is only ever launched (never recorded) needs no table line: k_op and crux_launch take any such struct.
#pragma once
#include "common.h"
#include <type_traits>
#include <vector>

// ---- the op table: the ONE list of the executor's ops -------------------------------------------------------------------------------------
// X(id, op type, tail): tail = 1 when the body may run as the sequential tail of a one-block op (the loss heads that consume a target; see k_phase_k).
// S(id, op type): an entry whose dispatch is written by hand beside the generated switch (exec.hip says why). The enumerators number from 1 in this order.
#define CRUX_EXEC_OPS(X, S) \
  X(OP_GEMM, GemmOp, 0) X(OP_ACT_GRAD, ActGradOp, 0) X(OP_GAUSS_EXPLORE, GaussExploreOp, 0) X(OP_CONCAT_SA, ConcatSaOp, 0) X(OP_SAC_TARGET, SacTargetOp, 0) \
  X(OP_DPG_ACTION, DpgActionOp, 0) X(OP_DPG_TARGET, DpgTargetOp, 0) X(OP_FILL, FillOp, 0) X(OP_SLICE_ROWS, SliceRowsOp, 0) X(OP_MEAN_INFO, MeanInfoOp, 0) \
  X(OP_TEMP_HEAD, TempHeadOp, 0) X(OP_Q_HEAD, QHeadOp, 1) X(OP_TD_HEAD, TdHeadOp, 1) X(OP_TD_INFO, TdInfoOp, 0) X(OP_SUMSQ2, Sumsq2Op, 0) \
  X(OP_CRITIC_INFO, CriticInfoOp, 0) X(OP_ACTOR_HEAD, ActorHeadOp, 0) X(OP_ACTOR_GRAD, ActorGradOp, 0) X(OP_ROWSUM, RowsumOp, 0) X(OP_ACTOR_INFO, ActorInfoOp, 0) \
  X(OP_ADAM_GATED, AdamGatedOp, 0) X(OP_PER_SEARCH, PerSearchOp, 0) X(OP_UNIFORM_IDS, UniformIdsOp, 0) X(OP_GATHER_RING_ALL, GatherRingAllOp, 0) X(OP_RING_IDS, RingIdsOp, 0) \
  X(OP_LEAF_REFRESH, LeafRefreshOp, 0) X(OP_TREE_TOUCH, TreeTouchOp, 0) X(OP_PER_UPDATE, PerUpdateOp, 1) X(OP_DQN_TARGET, DqnTargetOp, 0) X(OP_TD_ERROR, TdErrorOp, 0) \
  X(OP_POLYAK, PolyakOp, 0) X(OP_COPY_F32, CopyF32Op, 0) X(OP_ADAM_ADVANCE, AdamAdvanceOp, 0) X(OP_SOFTQ_TARGET, SoftqTargetOp, 0) \
  X(OP_FWD12, Fwd12Op, 0) X(OP_WGRAD2, Wgrad2Op, 0) S(OP_DGRAD2W1, Dgrad2W1Op)                                /* dense_fused.h (round 4) */ \
  S(OP_PER_SAMPLE, PerSampleGatherOp)                                  /* per.hip: search + gather of one row per wave (round 4) */ \
  X(OP_ACTOR_EXPLORE_TILE, ActorExploreTileOp, 0) X(OP_SAC_CRITIC_TILE, SacCriticTileOp, 0) X(OP_CRITIC_INFO2, CriticInfo2Op, 0) X(OP_SAC_ACTOR_TILE, SacActorTileOp, 0) \
  X(OP_ACTOR_INFO2, ActorInfo2Op, 0) X(OP_CRITIC_DX_TILE, CriticDxActorGradTileOp, 0) X(OP_DQN_TD_TILE, DqnTdTileOp, 0) X(OP_TD_INFO2, TdInfo2Op, 0)     /* sac_fused.h (round 4) */ \
  X(OP_LEAF_TOUCH, LeafTouchOp, 0)                                     /* per.hip: leaf re-sum + root paths in one launch (round 4) */ \
  X(OP_ADAM_SELF, AdamSelfOp, 0) X(OP_ADAM_ADVANCE_SELF, AdamAdvanceSelfOp, 0)      /* sac.hip: Adam gated on the producers' NaN flags, in the phase of the norm (round 4) */ \
  X(OP_SIGMA_EXPLORE, SigmaExploreOp, 0) X(OP_SIGMA_ACTOR_GRAD, SigmaActorGradOp, 0)      /* sac.hip: two-headed Gaussian actors; they take OP_GAUSS_EXPLORE's / OP_ACTOR_GRAD's phases */

#define EXEC_OP_ENUM(id, ...) id,
enum { OP_NONE = 0 /* an unused slot of a phase record */, CRUX_EXEC_OPS(EXEC_OP_ENUM, EXEC_OP_ENUM) };
// op type -> id. Declared from forward declarations: the translation units outside the off-policy unit see only the op structs they launch (ops_small.h).
template <class Op> struct OpKid;      // no definition: an op type that is not in the table cannot be recorded
#define EXEC_OP_KID(id, Op, ...) struct Op; template <> struct OpKid<Op> { static constexpr int value = id; };
CRUX_EXEC_OPS(EXEC_OP_KID, EXEC_OP_KID)
// may the op run as a sequential tail (PH_SEQ_TAIL)? The in-block tail switch of the phase kernels is generated from the same column.
#define EXEC_OP_TAIL(id, Op, tail) case id: return tail != 0;
#define EXEC_OP_SKIP(...)
static inline bool exec_op_tail(int kid) { switch (kid) { CRUX_EXEC_OPS(EXEC_OP_TAIL, EXEC_OP_SKIP) default: return false; } }

#define CRUX_EXEC_ARG_BYTES 768
struct ExecOp { int32_t kid; uint32_t nblocks; int32_t barrier; int32_t abytes; alignas(8) unsigned char args[CRUX_EXEC_ARG_BYTES]; };   // abytes: size of the packed arguments actually used

// ---- argument packs: the parameters of XOp::run after (bid, nblocks), stored by value in declaration order --------------------------------
template <class... T> struct ArgPack;
template <> struct ArgPack<> { __host__ __device__ ArgPack() {} };
template <class H, class... T> struct ArgPack<H, T...> {
  H head; ArgPack<T...> tail;
  __host__ __device__ ArgPack() {}
  __host__ __device__ ArgPack(H h, T... t) : head(h), tail(t...) {}
};
template <class F> struct OpSig;
template <class... A> struct OpSig<void (*)(const unsigned, const unsigned, A...)> { using pack = ArgPack<std::remove_cv_t<A>...>; };
template <class Op> using OpPack = typename OpSig<decltype(&Op::run)>::pack;

template <class Op, class... Done> __device__ __forceinline__ void exec_apply(unsigned bid, unsigned nb, const ArgPack<>&, Done... d) { Op::run(bid, nb, d...); }
template <class Op, class H, class... T, class... Done> __device__ __forceinline__ void exec_apply(unsigned bid, unsigned nb, const ArgPack<H, T...>& p, Done... d) {
  exec_apply<Op>(bid, nb, p.tail, d..., p.head);
}

// ---- host: recording --------------------------------------------------------------------------------------------------------------------
struct ExecReadback { float* host_info; const float* d_info; const int32_t* d_status; const char* who; };
struct ExecRec {
  std::vector<ExecOp> ops;
  bool active = false;
  char* small = nullptr; size_t small_cap = 0, small_off = 0;     // device: the recorded steps' info rows / statistics / status words, valid until the read-back
  std::vector<ExecReadback> readbacks;
  void* d_ops = nullptr; size_t d_ops_cap = 0;                     // device copy of the op list
  void* h_stage = nullptr; size_t h_stage_cap = 0;                 // pinned staging of the op list and of the read-backs
  size_t scratch_floor = 0, scratch_off = 0;                       // scratch requests made while recording are carved one after the other from the pre-sized block
  // chained epochs (run_epoch_chains in exec.hip: crux_dqn_epochs, crux_sac_epochs, crux_dpg_epochs and their asynchronous forms): several value_training epochs recorded
  // into ONE list, scheduled and run once -- no host round trip between the epochs of an iteration. While `chain` is set the per-epoch recorders append their phase tags
  // (offset by chain_base, see EpochTags) instead of scheduling and running; chain_ok = false sends the list through unscheduled.
  bool chain = false, chain_ok = true; int chain_base = 0; std::vector<int> chain_tags;
  // asynchronous runs (crux_*_epochs_async): no read-back, no host synchronisation -- the info rows are copied to a caller-owned device array by ops of the list itself.
  // The op list is uploaded from a ring of pinned staging buffers, so the host may record and enqueue up to three chains ahead of the one the device is running.
  bool async = false;
  float* info_row_override = nullptr;      // asynchronous tile-plan epochs: the epoch's info op writes the caller's device row itself (no copy op, no extra phase behind the chain's last epoch)
  void* h_ring[4] = {nullptr, nullptr, nullptr, nullptr}; size_t h_ring_cap[4] = {0, 0, 0, 0}; void* h_ring_ev[4] = {nullptr, nullptr, nullptr, nullptr}; unsigned h_ring_next = 0;
};
bool crux_exec_recording(const crux_ctx* c);
int32_t crux_exec_begin(crux_ctx* c);                 // start recording on this context (the launch sites below push ops instead of launching)
int32_t crux_exec_run(crux_ctx* c);                   // upload, launch the phases, fulfil the recorded read-backs; ends the recording
void crux_exec_abort(crux_ctx* c);                    // drop a recording after an error
ExecOp* crux_exec_new_op(crux_ctx* c, int kid, unsigned nblocks);
void* crux_exec_small(crux_ctx* c, size_t bytes);     // 256-byte aligned block of the small region (valid until the next crux_exec_begin)
void crux_exec_add_readback(crux_ctx* c, float* host_info, const float* d_info, const int32_t* d_status, const char* who);

template <class Op, class... A> inline void crux_exec_push(crux_ctx* c, unsigned nblocks, A... a) {
  using P = OpPack<Op>;
  ExecOp* op = crux_exec_new_op(c, OpKid<Op>::value, nblocks);
  P p(a...);
  memcpy(op->args, &p, sizeof p); op->abytes = (int32_t)sizeof p;
}
// ---- the stand-alone kernel of an op: the same body, one block of the grid per bid -----------------------------------------------------------
// An op struct may state `static constexpr int max_threads` (the kernel's __launch_bounds__); without it the kernel is compiled for HIP's default of 1024.
template <class Op, class = void> struct OpMaxThreads { static constexpr int value = 1024; };
template <class Op> struct OpMaxThreads<Op, std::void_t<decltype(Op::max_threads)>> { static constexpr int value = Op::max_threads; };
template <class Op, int MaxThreads, class... A> __global__ __launch_bounds__(MaxThreads) void k_op(A... a) { Op::run(blockIdx.x, gridDim.x, a...); }
template <class Op, class Pack = OpPack<Op>> struct OpLaunch;
template <class Op, class... P> struct OpLaunch<Op, ArgPack<P...>> {      // (P: the parameter types of Op::run, so the call converts its arguments as a direct call would)
  static void go(unsigned nblocks, unsigned nt, hipStream_t stream, P... p) { hipLaunchKernelGGL((k_op<Op, OpMaxThreads<Op>::value, P...>), dim3(nblocks), dim3(nt), 0, stream, p...); }
};
// a plain launch of an op's kernel (never recorded), for any op struct -- in the executor's table or not
template <class Op, class... A> inline void crux_launch(unsigned nblocks, unsigned nt, hipStream_t stream, A... a) { OpLaunch<Op>::go(nblocks, nt, stream, a...); }
// a launch site: record when the context is recording, launch otherwise. NT = threads per block of the stand-alone launch (the phase kernels always run 256).
#define CRUX_RUN(c, OpT, nblocks, NT, stream, ...)                                                            \
  do { if (crux_exec_recording(c)) crux_exec_push<OpT>((c), (unsigned)(nblocks), __VA_ARGS__);                  \
       else crux_launch<OpT>((unsigned)(nblocks), NT, (stream), __VA_ARGS__); } while (0)
// hipMemsetAsync(p, 0, bytes) of Float32 data inside a recordable chain
int32_t crux_exec_zero(crux_ctx* c, void* d_ptr, size_t bytes, hipStream_t st);
