// exec.hip -- the fused-step executor (see exec.h) and the fused value_training epochs built on it. Part of the off-policy unit
// (offpolicy_unit.hip includes dense.hip, sac.hip, per.hip and this file, so that one translation unit sees every op body).
#include "exec.h"
#include "ops_small.h"
#include <algorithm>

#define EXEC_SMALL_BYTES (256 * 1024)

// ---- device: the phase kernels ------------------------------------------------------------------------------------------------------------
// an op body with its record read where it lies, at a uniform address (scalar loads). Rec: an ExecOp of the list in global memory (k_phase), or a KOp naming a
// record inside the kernel arguments (k_phase_k)
template <class Op, class Rec> __device__ __forceinline__ void exec_dispatch(const Rec* op, unsigned bid) {
  const OpPack<Op> p = *(const OpPack<Op>*)op->args;
  exec_apply<Op>(bid, op->nblocks, p);
}
// The dispatch of a phase kernel, generated from the op table (exec.h): `kid`, `op` and `b` are the caller's. Two entries are written by hand:
//   OP_PER_SAMPLE reads its arguments through a pointer (PerSampleGatherOp::run_ptr: a by-value copy of the column table would live in scratch);
//   OP_DGRAD2W1 is compiled into the EXEC_HEAVY instantiations only (~300 VGPRs: see k_phase), in the form the phase needs.
#define EXEC_CASE(id, Op, tail) case id: exec_dispatch<Op>(op, b); break;
#define EXEC_SWITCH \
      switch (kid) { \
        CRUX_EXEC_OPS(EXEC_CASE, EXEC_OP_SKIP) \
        case OP_PER_SAMPLE: PerSampleGatherOp::run_ptr(b, op->nblocks, (const PerSampleArgs*)op->args); break; \
        case OP_DGRAD2W1: if constexpr (EXEC_HEAVY == 1) { exec_dispatch<Dgrad2W1OpT<1>>(op, b); } else if constexpr (EXEC_HEAVY == 2) { exec_dispatch<Dgrad2W1Op>(op, b); } break; \
        default: break; \
      }
// the ops that may run as the sequential tail of a one-block op (the table's tail column; exec_schedule refuses any other with exec_op_tail): a small switch of its
// own, so that the main dispatch stays straight-line (with the full switch inside a loop every phase ran ~1 us longer)
#define EXEC_CASE_TAIL_0(id, Op)
#define EXEC_CASE_TAIL_1(id, Op) case id: exec_dispatch<Op>(op, b); break;
#define EXEC_CASE_TAIL(id, Op, tail) EXEC_CASE_TAIL_##tail(id, Op)
#define EXEC_SWITCH_TAIL \
      switch (kid) { \
        CRUX_EXEC_OPS(EXEC_CASE_TAIL, EXEC_OP_SKIP) \
        default: break; \
      }
// every op of the table has a body, and its arguments fit an ExecOp as plain data
#define EXEC_OP_CHECK(id, Op, ...) static_assert(sizeof(OpPack<Op>) <= CRUX_EXEC_ARG_BYTES, #Op ": arguments exceed the ExecOp slot"); \
                                   static_assert(std::is_trivially_copyable<OpPack<Op>>::value, #Op ": arguments must be plain data");
CRUX_EXEC_OPS(EXEC_OP_CHECK, EXEC_OP_CHECK)

// One PHASE of a recorded sequence as one launch over the whole chip: block x of the grid belongs to the op whose block range contains x. The ops of a
// phase do not depend on each other, the dependency between phases is the kernel boundary -- no in-kernel barrier, no coherence question, all 256 CUs.
// A fused epoch then costs (number of phases) launches instead of (number of kernels): 13 instead of 25 for a DQN epoch, 30 instead of ~75 for SAC (10 / 27 per epoch inside a chain).
// EXEC_HEAVY: the register-hungry op bodies (Dgrad2W1Op: ~300 VGPRs) are compiled into the HEAVY instantiations only; a phase without such an op runs the light
// kernel (~100 VGPRs: four workgroups per CU instead of one -- a phase of 500-800 light blocks then takes one round over the chip instead of three)
__global__ __launch_bounds__(256) void k_phase(const ExecOp* __restrict__ ops, int n) {
  constexpr int EXEC_HEAVY = 2;
  // ops flagged sequential (barrier bit 1) own no blocks: they run in the block of the op before them, after it (see k_phase_k)
  unsigned b = blockIdx.x; int o = 0;
  for (;;) { const unsigned nb = (ops[o].barrier & 2) ? 0u : ops[o].nblocks; if (o + 1 < n && b >= nb) { b -= nb; ++o; } else break; }
  { const ExecOp* op = ops + o; const int kid = op->kid;
    EXEC_SWITCH }
  while (o + 1 < n && (ops[o + 1].barrier & 2)) { __threadfence(); __syncthreads(); ++o; b = 0;
    const ExecOp* op = ops + o; const int kid = op->kid;
    EXEC_SWITCH_TAIL }
}
// The same phase with its op records INSIDE the kernel arguments (<= 8 ops, <= 3.8 KB of packed arguments: every phase of the DQN / SAC epochs). With the records in
// global memory a workgroup walks block counts -> body id -> arguments -> the op's own data: three dependent scalar loads from memory the host copy has just written
// (cold in every cache) before the first useful load, ~4 us of a one-block phase's 6. The kernel-argument segment is read once, by independent scalar loads, so the
// chain is arguments -> data, as in a stand-alone launch.
// The argument struct comes in three sizes (the host copies it on every launch: with 4 KB per launch the enqueue, not the GPU, paced a SAC epoch).
#define PHASEK_MAXOPS 14
#define PHASEK_SEQ 0x10000
template <int BYTES> struct PhaseK { int32_t n; int32_t pad; int32_t kid[PHASEK_MAXOPS]; uint32_t nblocks[PHASEK_MAXOPS]; uint32_t off[PHASEK_MAXOPS]; alignas(16) unsigned char args[BYTES]; };
static_assert(sizeof(PhaseK<3840>) <= 4096, "HIP kernel arguments are limited to 4 KB");
struct KOp { const unsigned char* args; unsigned nblocks; };
// the gather's column table (456 bytes) is read where it lies in the kernel arguments instead of travelling by value (see GatherRingAllOp::run_ptr)
template <> __device__ __forceinline__ void exec_dispatch<GatherRingAllOp, KOp>(const KOp* op, unsigned bid) {
  using P = OpPack<GatherRingAllOp>; const P* pp = (const P*)op->args;
  GatherRingAllOp::run_ptr(bid, op->nblocks, &pp->head, pp->tail.head, pp->tail.tail.head, pp->tail.tail.tail.head, pp->tail.tail.tail.tail.head);
}
// the same for the fused prioritized search + gather (its arguments carry the same table: taking the address of a by-value copy put 176 bytes of every thread into scratch,
// on the one phase of a C3 epoch that is a chain of dependent memory round trips; round 6)
template <> __device__ __forceinline__ void exec_dispatch<PerSampleGatherOp, KOp>(const KOp* op, unsigned bid) {
  PerSampleGatherOp::run_ptr(bid, op->nblocks, &((const OpPack<PerSampleGatherOp>*)op->args)->head);
}
template <int BYTES, int EXEC_HEAVY>
__global__ __launch_bounds__(256) void k_phase_k(PhaseK<BYTES> by_value) {
  // read through the kernel-argument segment pointer, not through the by-value parameter: indexing the parameter at a run-time offset would make the compiler
  // copy the aggregate to private memory first
  const PhaseK<BYTES>* pk = (const PhaseK<BYTES>*)__builtin_amdgcn_kernarg_segment_ptr();
  unsigned b = blockIdx.x; int o = 0; const int n = pk->n;
#pragma unroll
  for (int q = 0; q < PHASEK_MAXOPS - 1; ++q) { const unsigned nb = pk->nblocks[q]; const bool adv = o == q && q + 1 < n && b >= nb; b -= adv ? nb : 0u; o += adv ? 1 : 0; }
  // Sequential ops (kid flagged PHASEK_SEQ; block count 0 in the table above, so no block starts on them) run in the block of the op before them, after it: a one-block
  // op whose only consumer is another one-block op (target -> loss head) shares its launch instead of paying a kernel boundary (~5 us) for a 128-float hand-over.
  // Same compute unit, write-through L1: the fence + workgroup barrier make the first op's global stores visible to the second.
  { const int kid = pk->kid[o]; const KOp kop{pk->args + pk->off[o], pk->nblocks[o]}; const KOp* op = &kop;
    EXEC_SWITCH }
  while (o + 1 < n && (pk->kid[o + 1] & PHASEK_SEQ)) { __threadfence(); __syncthreads(); ++o; b = 0;
    const int kid = pk->kid[o] & (PHASEK_SEQ - 1); const KOp kop{pk->args + pk->off[o], 1u}; const KOp* op = &kop;
    EXEC_SWITCH_TAIL }
}
// host: pack ops [i0, i1] of a recording into a PhaseK<BYTES>; false when they do not fit
template <int BYTES> static bool phasek_launch(const std::vector<ExecOp>& ops, size_t i0, size_t i1, unsigned blocks, hipStream_t st) {
  PhaseK<BYTES> pk; pk.n = 0; pk.pad = 0; size_t used = 0;
  for (size_t i = i0; i <= i1; ++i) { const ExecOp& e = ops[i]; if (!e.nblocks) continue;
    const size_t raw = (size_t)(e.abytes > 0 ? e.abytes : CRUX_EXEC_ARG_BYTES), ab = (raw + 15) & ~(size_t)15;
    if (pk.n >= PHASEK_MAXOPS || used + ab > (size_t)BYTES) return false;
    const bool seq = (e.barrier & 2) != 0;
    pk.kid[pk.n] = e.kid | (seq ? PHASEK_SEQ : 0); pk.nblocks[pk.n] = seq ? 0u : e.nblocks; pk.off[pk.n] = (uint32_t)used; memcpy(pk.args + used, e.args, raw); used += ab; pk.n++; }
  if (pk.n == 0) return false;
  for (int q = pk.n; q < PHASEK_MAXOPS; ++q) { pk.kid[q] = 0; pk.nblocks[q] = 0; pk.off[q] = 0; }
  int heavy = 0;      // 0: no Dgrad2W1Op in the phase; 1: its O3 = 1 form (critics / no folded output layer); 2: the O3 = 4 form
  for (int q = 0; q < pk.n; ++q) if ((pk.kid[q] & (PHASEK_SEQ - 1)) == OP_DGRAD2W1) { Dgrad2Args a; memcpy(&a, pk.args + pk.off[q], sizeof a); heavy = std::max(heavy, (a.z.W3 && a.z.out3 > 1) ? 2 : 1); }
  if (heavy == 2) hipLaunchKernelGGL((k_phase_k<BYTES, 2>), dim3(blocks), dim3(256), 0, st, pk);
  else if (heavy == 1) hipLaunchKernelGGL((k_phase_k<BYTES, 1>), dim3(blocks), dim3(256), 0, st, pk);
  else hipLaunchKernelGGL((k_phase_k<BYTES, 0>), dim3(blocks), dim3(256), 0, st, pk);
  return true;
}
// would phasek_launch<3840> take ops [i0, i1]? (the same packing rules, nothing launched)
static bool phasek_fits(const std::vector<ExecOp>& ops, size_t i0, size_t i1) {
  int n = 0; size_t used = 0;
  for (size_t i = i0; i <= i1; ++i) { const ExecOp& e = ops[i]; if (!e.nblocks) continue;
    const size_t raw = (size_t)(e.abytes > 0 ? e.abytes : CRUX_EXEC_ARG_BYTES), ab = (raw + 15) & ~(size_t)15;
    if (n >= PHASEK_MAXOPS || used + ab > (size_t)3840) return false;
    used += ab; ++n; }
  return n > 0;
}
// ---- host: recording -------------------------------------------------------------------------------------------------------------------
static ExecRec* rec_of(crux_ctx* c) { return (ExecRec*)c->rec; }
bool crux_exec_recording(const crux_ctx* c) { return c && c->rec && ((const ExecRec*)c->rec)->active; }
int32_t crux_exec_begin(crux_ctx* c) {
  if (!c->rec) c->rec = new ExecRec();
  ExecRec* r = rec_of(c);
  if (r->active) return crux_fail(c, CRUX_EINVAL, "executor: a recording is already open on this context");
  if (!r->small) { if (hipMalloc(&r->small, EXEC_SMALL_BYTES) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "executor: small region"); r->small_cap = EXEC_SMALL_BYTES; }
  if (!crux_scratch(c, (size_t)32 << 20)) return crux_fail(c, CRUX_ENOMEM, "executor: scratch");     // pre-sized: the scratch block must not move while pointers into it are recorded
  r->scratch_floor = c->scratch_bytes; r->scratch_off = 0;
  r->ops.clear(); r->readbacks.clear(); r->small_off = 0; r->active = true;
  r->chain_tags.clear(); r->chain_base = 0; r->chain_ok = true;
  return CRUX_OK;
}
// frees everything a context's executor ever allocated (called by crux_ctx_destroy after the stream has drained)
void crux_exec_destroy(crux_ctx* c) {
  if (!c || !c->rec) return;
  ExecRec* r = rec_of(c);
  if (r->small) (void)hipFree(r->small);
  if (r->d_ops) (void)hipFree(r->d_ops);
  if (r->h_stage) (void)hipHostFree(r->h_stage);
  for (int k = 0; k < 4; ++k) { if (r->h_ring[k]) (void)hipHostFree(r->h_ring[k]); if (r->h_ring_ev[k]) (void)hipEventDestroy((hipEvent_t)r->h_ring_ev[k]); }
  delete r; c->rec = nullptr;
}
void crux_exec_abort(crux_ctx* c) { if (c->rec) { ExecRec* r = rec_of(c); r->active = false; r->ops.clear(); r->readbacks.clear(); } }
ExecOp* crux_exec_new_op(crux_ctx* c, int kid, unsigned nblocks) {
  ExecRec* r = rec_of(c); r->ops.emplace_back(); ExecOp* op = &r->ops.back();
  op->kid = kid; op->nblocks = nblocks; op->barrier = 1; op->abytes = 0; return op;
}
void* crux_exec_scratch(crux_ctx* c, size_t bytes) {
  ExecRec* r = rec_of(c); bytes = (bytes + 255) / 256 * 256;
  if (r->scratch_off + bytes > r->scratch_floor) return nullptr;
  void* p = (char*)c->scratch + r->scratch_off; r->scratch_off += bytes; return p;
}
void* crux_exec_small(crux_ctx* c, size_t bytes) {
  ExecRec* r = rec_of(c); bytes = (bytes + 255) / 256 * 256;
  if (!r || r->small_off + bytes > r->small_cap) return nullptr;
  void* p = r->small + r->small_off; r->small_off += bytes; return p;
}
void crux_exec_add_readback(crux_ctx* c, float* host_info, const float* d_info, const int32_t* d_status, const char* who) { rec_of(c)->readbacks.push_back({host_info, d_info, d_status, who}); }
int32_t crux_exec_zero(crux_ctx* c, void* d_ptr, size_t bytes, hipStream_t st) {
  if (!crux_exec_recording(c)) { HIPCHK(c, hipMemsetAsync(d_ptr, 0, bytes, st)); return CRUX_OK; }
  if (bytes % 4) return crux_fail(c, CRUX_EINVAL, "executor: zero-fill of %zu bytes", bytes);
  const int64_t n = (int64_t)(bytes / 4);
  crux_exec_push<FillOp>(c, (unsigned)((n + 255) / 256), (float*)d_ptr, 0.f, n);
  return CRUX_OK;
}
// Phases: ops that do not depend on each other share a barrier. The caller assigns every recorded op a phase number (non-decreasing along every
// dependency chain); the list is stably sorted by phase and only the last op of a phase keeps its barrier.
// Tags are 4 * phase + sub: sub 0 = an ordinary op of the phase; sub 1 = head of a sequential group, sorted behind the ordinary ops; sub 2 = runs in the block of
// the op sorted before it, after it (both must be one-block ops: the caller only tags such pairs -- PH_SEQ_HEAD / PH_SEQ_TAIL below).
static int32_t exec_schedule(crux_ctx* c, const std::vector<int>& phase) {
  ExecRec* r = rec_of(c); const size_t n = r->ops.size();
  if (phase.size() != n) return crux_fail(c, CRUX_EHIP, "executor: %zu phase tags for %zu ops", phase.size(), n);
  std::vector<size_t> idx(n); for (size_t i = 0; i < n; ++i) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return phase[a] < phase[b]; });
  std::vector<ExecOp> out(n);
  for (size_t k = 0; k < n; ++k) { out[k] = r->ops[idx[k]]; out[k].barrier = (k + 1 == n || (phase[idx[k + 1]] >> 2) != (phase[idx[k]] >> 2)) ? 1 : 0;
    if ((phase[idx[k]] & 3) == 2) {
      // the in-block tail switch (EXEC_SWITCH_TAIL) knows the table's tail ops only: anything else would be skipped silently
      if (!exec_op_tail(out[k].kid)) return crux_fail(c, CRUX_EHIP, "executor: op %d cannot run as a sequential tail", out[k].kid);
      if (k == 0 || (phase[idx[k - 1]] >> 2) != (phase[idx[k]] >> 2) || out[k].nblocks != 1 || out[k - 1].nblocks != 1) return crux_fail(c, CRUX_EHIP, "executor: a sequential op without a one-block predecessor in its phase");
      out[k].barrier |= 2; } }
  r->ops.swap(out); return CRUX_OK;
}
// launches of the dense engine inside a recorded chain: a tile GEMM, or one of the fused block kernels of dense_fused.h (round 4). The phase plans below count THESE
// in recording order; a network's forward pass is nf of them (nf = L, or L - 1 when layers 0 + 1 are one Fwd12Op), its pullback with parameter gradients 2 L - 1
// (weight + data gradient per layer, no data gradient for layer 0) in L phases -- or 2 (L - 1) in L - 1 phases when Wgrad2Op || Dgrad2W1Op take layers 1 and 0 together.
static inline bool is_mm(int kid) { return kid == OP_GEMM || kid == OP_FWD12 || kid == OP_WGRAD2 || kid == OP_DGRAD2W1; }
// With the output layer's data gradient folded into the pair (three layers, out <= 4: crux_dense_bwd_fused3) the whole pullback is ONE phase of three launches
// (output-layer dW, Wgrad2Op, Dgrad2W1Op), and an input-gradient chain is two (Dgrad2W1Op, layer 0's data gradient).
struct NetPlan { int nf, nbops, nb, dq; bool one; int stage(int k) const { return one ? 0 : k / 2; } };
static inline NetPlan net_plan(const crux_mlp* n, int64_t B) { const int L = n->nd.L; const bool ff = crux_dense_fwd_fused(n), fb = crux_dense_bwd_fused(n, B), f3 = crux_dense_bwd_fused3(n, B);
  return NetPlan{ff ? L - 1 : L, f3 ? 3 : fb ? 2 * (L - 1) : 2 * L - 1, f3 ? 1 : fb ? L - 1 : L, f3 ? 2 : L, f3}; }
#define PH_SEQ_HEAD (1 << 12)
#define PH_SEQ_TAIL (2 << 12)
static inline int ph_tag(int p_mapped, int sub) { return 4 * p_mapped + sub; }
// What the generic SAC and DDPG / TD3 epoch plans share (SacRun::one, DpgRun::one draw the phase tables). Written in launches: FA / FQ forward launches of the actor / a
// critic, BQ / BA phases of a pullback with parameter gradients (BQo ops per critic), DQ phases of a critic's input-gradient chain; with the fused block kernels FA = FQ = L - 1
// and BQ = BA = L - 1 (net_plan above), otherwise all equal L. X = the target's phase, Y = the first phase of the actor step's critic passes. sq: the target (one block at
// B <= 256) and the critic heads (one block each) form a sequential group in ONE block of phase X when the critics train; the critic chain and all behind it (Y ..) sit one earlier.
struct ActorCriticPlan {
  NetPlan pa, pq; int64_t B; int LA, LQ, FA, FQ, BQ, BQo, BA, DQ, sq, X, Y;
  ActorCriticPlan(const crux_mlp* actor, const crux_mlp* q1, int64_t B_, bool update_critic) : pa(net_plan(actor, B_)), pq(net_plan(q1, B_)), B(B_), LA(actor->nd.L), LQ(q1->nd.L),
    FA(pa.nf), FQ(pq.nf), BQ(pq.nb), BQo(pq.nbops), BA(pa.nb), DQ(pq.dq), sq((update_critic && B_ <= 256) ? 1 : 0), X(3 + FA + FQ), Y(X + 4 + BQ - sq) {}
  // the plan holds for networks of one depth and one launch count: the second critic (NULL: none) like the first, the target critics' forward passes like a critic's
  bool ok(const crux_mlp* q2, const crux_mlp* q1t, const crux_mlp* q2t) const {
    if (LA != LQ || FA != FQ || q1t->nd.L != LQ || net_plan(q1t, B).nf != FQ) return false;
    if (q2 && (q2->nd.L != LQ || net_plan(q2, B).nf != FQ || net_plan(q2, B).nb != BQ)) return false;
    return !(q2t && (q2t->nd.L != LQ || net_plan(q2t, B).nf != FQ)); }
  // rand!: 0 ids | 1 gather
  static int sampling(int kid) { return kid == OP_UNIFORM_IDS ? 0 : kid == OP_GATHER_RING_ALL ? 1 : -1; }
  // the target: 2.. actor(sp) forward | 2+FA the next action (action_op) | 3+FA.. target Q1 || Q2 forward | X the target itself (target_op), head of the sequential group
  int target(int kid, int& g, int action_op, int target_op) const {
    if (is_mm(kid)) { const int k = g++; return k < FA ? 2 + k : 3 + FA + (k - FA) % FQ; }
    return kid == action_op ? 2 + FA : kid == target_op ? X | (sq ? PH_SEQ_HEAD : 0) : -1; }
  // the critic step, per critic: FQ forward launches, head, then (weight, data) pairs from the last layer down (the first layer has no data gradient)
  int critic(int kid, int& g) const {
    if (kid == OP_FILL) return 1; if (kid == OP_CONCAT_SA) return 2;
    if (is_mm(kid)) { const int k = (g++) % (FQ + BQo); return k < FQ ? 3 + k : X + 2 - sq + pq.stage(k - FQ); }
    return kid == OP_Q_HEAD ? (sq ? (X | PH_SEQ_TAIL) : X + 1) : kid == OP_SUMSQ2 ? X + 2 - sq + BQ : (kid == OP_CRITIC_INFO || kid == OP_ADAM_GATED) ? X + 3 - sq + BQ : kid == OP_ADAM_ADVANCE ? X + 4 - sq + BQ : -1; }
};

int32_t crux_exec_run(crux_ctx* c) {
  ExecRec* r = rec_of(c);
  if (!r || !r->active) return crux_fail(c, CRUX_EINVAL, "executor: no open recording");
  r->active = false;
  if (c->scratch_bytes != r->scratch_floor) return crux_fail(c, CRUX_EHIP, "executor: the scratch block moved while it was being recorded");
  const size_t nops = r->ops.size();
  int32_t rc = CRUX_OK;
  if (nops) {
    const size_t ob = nops * sizeof(ExecOp), rb = r->readbacks.size() * (sizeof(float) * CRUX_INFO_N + 16), need_h = ob + rb;
    if (r->d_ops_cap < ob) { if (r->d_ops) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(r->d_ops); } r->d_ops_cap = ob * 2 + 4096; if (hipMalloc(&r->d_ops, r->d_ops_cap) != hipSuccess) { r->d_ops = nullptr; r->d_ops_cap = 0; return crux_fail(c, CRUX_ENOMEM, "executor: op list"); } }
    const bool async = r->async; r->async = false;
    void* stage = nullptr;
    r->ops.back().barrier &= 2;
    // an asynchronous chain whose phases all travel in kernel arguments needs no device copy of the list: one stream operation less between chains (it sits IN the
    // stream there)
    bool lean = false;
    if (async && !crux_sw().exec_no_kernarg) { lean = true;
      size_t i0 = 0;
      while (i0 < nops && lean) { size_t i1 = i0; unsigned blocks = 0; for (;;) { blocks += (r->ops[i1].barrier & 2) ? 0u : r->ops[i1].nblocks; if ((r->ops[i1].barrier & 1) || i1 + 1 == nops) break; ++i1; }
        if (blocks && !phasek_fits(r->ops, i0, i1)) lean = false;
        i0 = i1 + 1; } }
    if (lean) { /* nothing to upload */ }
    else if (async) {      // a staging buffer of its own for this chain: the previous chains' uploads may not have executed yet
      const unsigned k = r->h_ring_next++ & 3u;
      if (!r->h_ring_ev[k]) { hipEvent_t ev; HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming)); r->h_ring_ev[k] = ev; }
      else HIPCHK(c, hipEventSynchronize((hipEvent_t)r->h_ring_ev[k]));      // the upload that last used this buffer (four chains ago) has run
      if (r->h_ring_cap[k] < ob) { if (r->h_ring[k]) (void)hipHostFree(r->h_ring[k]); r->h_ring_cap[k] = ob * 2 + 4096;
        if (hipHostMalloc(&r->h_ring[k], r->h_ring_cap[k], hipHostMallocDefault) != hipSuccess) { r->h_ring[k] = nullptr; r->h_ring_cap[k] = 0; return crux_fail(c, CRUX_ENOMEM, "executor: staging ring"); } }
      stage = r->h_ring[k];
      memcpy(stage, r->ops.data(), ob);
      HIPCHK(c, hipMemcpyAsync(r->d_ops, stage, ob, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipEventRecord((hipEvent_t)r->h_ring_ev[k], c->stream));
    } else {
    if (r->h_stage_cap < need_h) { if (r->h_stage) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipHostFree(r->h_stage); } r->h_stage_cap = need_h * 2 + 4096; if (hipHostMalloc(&r->h_stage, r->h_stage_cap, hipHostMallocDefault) != hipSuccess) { r->h_stage = nullptr; r->h_stage_cap = 0; return crux_fail(c, CRUX_ENOMEM, "executor: staging"); } }
    memcpy(r->h_stage, r->ops.data(), ob);
    HIPCHK(c, hipMemcpyAsync(r->d_ops, r->h_stage, ob, hipMemcpyHostToDevice, c->stream));
    }
    // one launch per phase over the whole chip (see k_phase); the phase's records travel in the kernel arguments when they fit (see k_phase_k; zero-block ops are dropped
    // there). DESIGN 4.3 has the numbers against the persistent one-XCD form this replaced.
    size_t i0 = 0;
    while (i0 < nops) { size_t i1 = i0; unsigned blocks = 0; for (;;) { blocks += (r->ops[i1].barrier & 2) ? 0u : r->ops[i1].nblocks; if ((r->ops[i1].barrier & 1) || i1 + 1 == nops) break; ++i1; }
      if (blocks) {
        const bool no_kernarg = crux_sw().exec_no_kernarg;      // tests: every phase through the global-record form
        if (no_kernarg || (!phasek_launch<384>(r->ops, i0, i1, blocks, c->stream) && !phasek_launch<1024>(r->ops, i0, i1, blocks, c->stream) && !phasek_launch<3840>(r->ops, i0, i1, blocks, c->stream)))
          hipLaunchKernelGGL(k_phase, dim3(blocks), dim3(256), 0, c->stream, (const ExecOp*)r->d_ops + i0, (int)(i1 - i0 + 1));
      }
      i0 = i1 + 1; }
    rc = crux_launch_check(c, "k_phase"); if (rc) return rc;
    if (async) { r->ops.clear(); r->readbacks.clear(); return CRUX_OK; }      // nothing is read back: the list itself copied the info rows where the caller wants them
    char* hb = (char*)r->h_stage + ob;
    for (size_t k = 0; k < r->readbacks.size(); ++k) { char* h = hb + k * (sizeof(float) * CRUX_INFO_N + 16);
      HIPCHK(c, hipMemcpyAsync(h, r->readbacks[k].d_info, sizeof(float) * CRUX_INFO_N, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(h + sizeof(float) * CRUX_INFO_N, r->readbacks[k].d_status, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream)); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < r->readbacks.size(); ++k) { const char* h = hb + k * (sizeof(float) * CRUX_INFO_N + 16);
      if (r->readbacks[k].host_info) memcpy(r->readbacks[k].host_info, h, sizeof(float) * CRUX_INFO_N);
      int32_t st; memcpy(&st, h + sizeof(float) * CRUX_INFO_N, sizeof st);
      if (st == CRUX_ENAN && !rc) rc = crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20) in %s", r->readbacks[k].who); }
  }
  r->ops.clear(); r->readbacks.clear();
  return rc;
}

// ---- fused value_training epochs ------------------------------------------------------------------------------------------------------------
int32_t crux_per_prepare(crux_buffer* source);      // per.hip: any full rebuild of the cumsum tree happens before the recording starts

// The phase tags of one recorded epoch. tag(rule) tags the ops recorded since the last tag by rule(kid, g) -> phase | PH_SEQ_* (g: a counter the rule may use,
// zero for every call); a miss (-1) sends the epoch through unscheduled. Inside a chain (ExecRec::chain) every phase moves to the chain's base: phases 0 and 1
// (the epoch's sampling) back by `lead`, every later phase back by `rest` -- the overlap with the epoch before. finish(len) ends an epoch of `len` phases: inside a
// chain its tags join the chain's, otherwise the list is scheduled and run. Without a recording (r = NULL: the epoch runs call by call) it does nothing.
struct EpochTags {
  crux_ctx* c; ExecRec* r; const char* who; int lead, rest, base = 0; size_t first = 0, m = 0; bool plan_ok = true; std::vector<int> ph;
  EpochTags(crux_ctx* c_, bool on, const char* who_, int lead_, int rest_) : c(c_), r(on ? rec_of(c_) : nullptr), who(who_), lead(lead_), rest(rest_) {
    if (r) { base = r->chain ? r->chain_base : 0; first = m = r->ops.size(); } }
  template <class Rule> void tag(Rule&& rule) {
    if (!r) return;
    int g = 0;
    for (size_t i = m; i < r->ops.size(); ++i) { int p = rule(r->ops[i].kid, g);
      if (p < 0) { if (crux_sw().verbose) fprintf(stderr, "[cruxhip] %s: op kind %d has no phase in the plan\n", who, r->ops[i].kid); plan_ok = false; p = 0; }
      const int sub = p >> 12; p &= 4095;
      ph.push_back(ph_tag(base > 0 ? base + p - (p < 2 ? lead : rest) : p, sub)); }
    m = r->ops.size(); }
  void only(int p) { tag([p](int, int&) { return p; }); }
  int32_t finish(int len) {
    if (!r) return CRUX_OK;
    if (r->chain) {      // the chain's driver (run_epoch_chains) schedules and runs the whole list
      if (!(plan_ok && ph.size() == r->ops.size() - first)) r->chain_ok = false;
      r->chain_tags.insert(r->chain_tags.end(), ph.begin(), ph.end()); r->chain_base += len - (r->chain_base > 0 ? rest : 0);
      return CRUX_OK; }
    if (plan_ok && ph.size() == r->ops.size()) { const int32_t rc = exec_schedule(c, ph); if (rc) { crux_exec_abort(c); return rc; } }
    return crux_exec_run(c); }
};

// value_training's epoch loop (off_policy.jl:69: `for epoch in 1:c_opt.epochs`) as chains of up to 8 epochs, each ONE recorded list: the epochs are recorded back to back
// (record(e) records epoch e, its phases following those of epoch e - 1), and the host schedules, uploads and launches once per chain. A prioritized source (per) also
// ends a chain where its replay tree needs a full rebuild, and is brought up to date before every chain. chain = false: epoch by epoch, each run on its own.
// d_rows (asynchronous runs): the caller's device array [n_epochs][nrows][CRUX_INFO_N]; rows(e) names the info rows epoch e registers (bit k: row k, in the order the
// steps ran) and the phase their copies join: `shift` phases after the epoch's last (tile plans: the info op sits IN the last phase), none for shift < 0 (the epoch's
// info op writes the caller's row itself). tail() records ops that join the last epoch's last phase (the DQN family's target update).
struct EpochRows { unsigned has; int shift; };
template <class Record, class Rows, class Tail>
static int32_t run_epoch_chains(crux_ctx* c, const char* who, bool chain, crux_buffer* per, int32_t n_epochs, int nrows, float* d_rows, Record&& record, Rows&& rows, Tail&& tail) {
  int32_t rc = CRUX_OK;
  if (!chain) { if (d_rows) return CRUX_EUNSUP;      // call by call, with a read-back per epoch: the caller takes the synchronous entry point
    for (int e = 0; e < n_epochs; ++e) { rc = record(e); if (rc) return rc; }
    return CRUX_OK; }
  auto fail = [&](int32_t e) { if (c->rec) rec_of(c)->chain = false; crux_exec_abort(c); return e; };
  auto flush = [&]() -> int32_t {
    if (!crux_exec_recording(c)) return CRUX_OK;
    ExecRec* r = rec_of(c); r->chain = false;
    if (r->chain_ok && r->chain_tags.size() == r->ops.size()) { const int32_t rs = exec_schedule(c, r->chain_tags); if (rs) { crux_exec_abort(c); return rs; } }
    r->async = d_rows != nullptr;
    return crux_exec_run(c);
  };
  size_t tg0 = 0;      // the first tag of the epoch recorded last
  auto last_phase = [&]() { const ExecRec* r = rec_of(c); int t = 0; for (size_t k = tg0; k < r->chain_tags.size(); ++k) t = std::max(t, r->chain_tags[k] & ~3); return t; };
  int in_chain = 0;
  for (int e = 0; e < n_epochs; ++e) {
    // a priority tree that needs a plain rebuild (the ring is still filling, or a bulk change) cannot be refreshed inside a recording: run what is recorded first
    if (in_chain && (in_chain >= 8 || (per && per->per_full_dirty))) { rc = flush(); in_chain = 0; if (rc) return rc; }
    if (!in_chain) { if (per) { rc = crux_per_prepare(per); if (rc) return rc; }
      rc = crux_exec_begin(c); if (rc) return rc; }
    ExecRec* r = rec_of(c); r->chain = true;
    const size_t rb0 = r->readbacks.size(); tg0 = r->chain_tags.size();
    rc = record(e); if (rc) return fail(rc);
    if (d_rows) {      // the epoch's info rows go to the caller's device array, copied in the epoch's last phase (one phase after the info ops wrote them)
      const EpochRows er = rows(e);
      if (!crux_exec_recording(c) || r->readbacks.size() != rb0 + (size_t)__builtin_popcount(er.has) || r->chain_tags.size() != r->ops.size())
        return fail(crux_fail(c, CRUX_EHIP, "%s epochs (async): unexpected recording", who));
      if (er.shift >= 0) { const int t = last_phase() + er.shift; size_t q = rb0;
        for (int k = 0; k < nrows; ++k) { if (!(er.has >> k & 1)) continue;
          crux_exec_push<CopyF32Op>(c, 1u, d_rows + ((size_t)e * nrows + k) * CRUX_INFO_N, (const float*)r->readbacks[q++].d_info, (int64_t)CRUX_INFO_N);
          r->chain_tags.push_back(t); } } }
    ++in_chain;
  }
  ExecRec* r = rec_of(c); const size_t n0 = r->ops.size();
  rc = tail(); if (rc) return fail(rc);
  if (r->ops.size() > n0) r->chain_tags.insert(r->chain_tags.end(), r->ops.size() - n0, last_phase());
  return flush();
}
// One value_training call of a family. Run (DqnRun, SacRun, DpgRun below) holds the call's networks, buffers, hyper-parameters, counters and epoch range, and offers valid()
// (the argument check: CRUX_EINVAL), chain(), per(), tail(), rows(e), shift(e) (what run_epoch_chains asks for) and epoch(e, host_rows), which records epoch e (call by call:
// runs it) with info row k going to host_rows[k] + e * CRUX_INFO_N. d_rows: the asynchronous form; otherwise host_rows[k]: host [n_epochs x CRUX_INFO_N] or NULL.
// More than one chain per call (n_epochs > 8, Run::ONE_READBACK): the chains run back to back in their asynchronous form, with the info rows in a device block of the
// context, and the host synchronises ONCE, at the end of the call: the device no longer idles while the host reads back, records and uploads the next chain (C4, 50
// epochs per call: 180 -> ~155 us per epoch). Same results; a NaN gradient norm is reported from the rows.
template <class Run> static int32_t run_family(const Run& run, float* const* host_rows, float* d_rows) {
  if (!run.valid()) return CRUX_EINVAL;
  crux_ctx* c = run.ctx(); constexpr int NR = Run::NROWS; const int32_t n_epochs = run.n_epochs;
  auto chains = [&](float* const* hr, float* dr) {
    return run_epoch_chains(c, Run::who, run.chain(), run.per(), n_epochs, NR, dr,
      [&](int e) {      // shift < 0, asynchronous: the epoch's info op writes the caller's row itself (no copy op)
        float* row = (dr && run.shift(e) < 0) ? dr + (size_t)e * NR * CRUX_INFO_N : nullptr;
        if (row) rec_of(c)->info_row_override = row;
        const int32_t rc = run.epoch(e, hr);
        if (row) rec_of(c)->info_row_override = nullptr;
        return rc; },
      [&](int e) { return EpochRows{run.rows(e), run.shift(e)}; }, [&] { return run.tail(); }); };
  static float* const none[NR] = {};
  if (d_rows) return chains(none, d_rows);
  if (!(Run::ONE_READBACK && n_epochs > 8 && run.chain() && !crux_sw().sync_chains)) return chains(host_rows, nullptr);
  const size_t need = sizeof(float) * NR * CRUX_INFO_N * (size_t)n_epochs;
  if (c->epoch_rows_bytes < need) { if (c->epoch_rows) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->epoch_rows); c->epoch_rows = nullptr; c->epoch_rows_bytes = 0; }
    if (hipMalloc(&c->epoch_rows, 2 * need) != hipSuccess) return crux_fail(c, CRUX_ENOMEM, "%s epochs: info rows", Run::who); c->epoch_rows_bytes = 2 * need; }
  HIPCHK(c, hipMemsetAsync(c->epoch_rows, 0, need, c->stream));
  const int32_t rc = chains(none, (float*)c->epoch_rows); if (rc) return rc;
  std::vector<float> rows((size_t)NR * CRUX_INFO_N * (size_t)n_epochs);
  HIPCHK(c, hipMemcpyAsync(rows.data(), c->epoch_rows, need, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  bool nan = false;
  for (int e = 0; e < n_epochs; ++e) { const unsigned h = run.rows(e);
    for (int k = 0; k < NR; ++k) { if (!(h >> k & 1)) continue;
      const float* row = rows.data() + ((size_t)e * NR + k) * CRUX_INFO_N;
      if (row[CRUX_INFO_GRAD_NORM] != row[CRUX_INFO_GRAD_NORM]) nan = true;
      if (host_rows[k]) memcpy(host_rows[k] + (size_t)e * CRUX_INFO_N, row, sizeof(float) * CRUX_INFO_N); } }
  if (nan) return crux_fail(c, CRUX_ENAN, "NaN detected! (grad norm is NaN, src/training.jl:20) in the %s epochs", Run::family);
  return CRUX_OK;
}
static inline float* info_row(float* const* host_rows, int k, int e) { return host_rows[k] ? host_rows[k] + (size_t)e * CRUX_INFO_N : nullptr; }
// c->epoch_tmp with at least `bytes` (targets and td errors of the epochs run call by call: a block of the context that no recording carves)
static int32_t grow_epoch_tmp(crux_ctx* c, size_t bytes, int64_t B, const char* who) {
  if (c->epoch_tmp_bytes >= bytes) return CRUX_OK;
  if (c->epoch_tmp) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->epoch_tmp); }
  c->epoch_tmp_bytes = 16 * (size_t)B + 4096;
  if (hipMalloc(&c->epoch_tmp, c->epoch_tmp_bytes) != hipSuccess) { c->epoch_tmp = nullptr; c->epoch_tmp_bytes = 0; return crux_fail(c, CRUX_ENOMEM, "%s: targets", who); }
  return CRUX_OK;
}
// softq_target(alpha) (rl/softq.jl:4-13). Lives in this translation unit so that the stand-alone kernel and the executor's phase kernel are compiled under the same
// floating-point contraction setting (exp / log are inlined library code: the two forms must agree bit for bit).
int32_t crux_mlp_forward_impl(crux_mlp* net, const float* d_x, int64_t B, float* d_y, const float* params_override);
extern "C" int32_t crux_softq_target(crux_mlp* tn, crux_buffer* batch, float gamma, float alpha, float* d_y) { CRUX_PLAIN_ONLY("crux_softq_target", tn);
  if (!tn || !batch || !d_y) return CRUX_EINVAL;
  crux_ctx* c = tn->ctx; const int64_t n = batch->elements; if (n == 0) return CRUX_OK;
  if (!(alpha > 0.f)) return crux_fail(c, CRUX_EINVAL, "softq_target: alpha must be positive");
  const int nout = tn->nd.dims[tn->nd.L];
  float* q = (float*)crux_scratch(c, 4 * (size_t)n * nout + 256); if (!q) return crux_fail(c, CRUX_ENOMEM, "softq_target: scratch");
  int32_t rc;
  if (tn->nd.maxdim >= CRUX_DENSE_MIN_WIDTH) { rc = crux_dense_forward(tn, (const float*)batch->col[CRUX_COL_SP], n, c->stream); if (rc) return rc; q = crux_dense_act(tn, tn->nd.L); }
  else { rc = crux_mlp_forward_impl(tn, (const float*)batch->col[CRUX_COL_SP], n, q, nullptr); if (rc) return rc; }
  CRUX_RUN(c, SoftqTargetOp, (unsigned)((n + 255) / 256), 256, c->stream, q, nout, (const float*)batch->col[CRUX_COL_R], (const uint8_t*)batch->col[CRUX_COL_DONE], gamma, alpha, n, d_y);
  return crux_launch_check(c, "k_softq_target");
}

extern "C" {
int32_t crux_per_sample(crux_buffer* target, crux_buffer* source, int64_t B, const double* rands, float beta, uint64_t i);
int32_t crux_uniform_sample(crux_buffer* target, crux_buffer* source, int64_t B, const int64_t* ids, uint64_t i);
int32_t crux_dqn_target(crux_mlp* tn, crux_buffer* batch, float gamma, float* d_y);
int32_t crux_td_step(crux_mlp* net, crux_buffer* batch, const float* d_y, int32_t use_weight, float* info_out);
int32_t crux_td_step_with_error(crux_mlp* net, crux_buffer* batch, const float* d_y, int32_t use_weight, float* d_err, float* info_out);
int32_t crux_per_update_device(crux_buffer* b, const int64_t* d_ids, const float* d_v, int64_t n);
int32_t crux_polyak(crux_mlp* to, const crux_mlp* from, float tau);

// The DQN-family epoch on the fused block kernels and DqnTdTileOp (sac_fused.h, round 4): 8 phases, FIVE launches per epoch inside a chain (round 3: 13 / 9).
//   0 [uniform ids] | 1 prioritized search + gather in one launch (or the gather), zero-fills | 2 layers 0+1 of Q(s) and Q-(s') | 3 both output layers + target + td head +
//   update_priorities! per 16-sample tile | 4 the whole pullback ; leaf re-sums | 5 norm ; root paths | 6 info, Adam | 7 beta-power advance
// In a chain the sampling of epoch e + 1 (phases 0, 1) sits beside the norm and Adam of epoch e -- after the root paths of phase 5 --, its phase 2 beside the advance.
// does the network pair take the recorded chain of crux_dqn_epochs* (wide enough for the dense engine; fused and chained epochs not switched off)?
static bool dqn_chain_case(const crux_mlp* net, const crux_mlp* tnet) { return net->nd.maxdim >= CRUX_DENSE_MIN_WIDTH && tnet->nd.maxdim >= CRUX_DENSE_MIN_WIDTH && !crux_sw().no_fused_epoch && !crux_sw().no_chained_epochs; }
static bool dqn_tile_case(crux_mlp* net, crux_mlp* tnet, crux_buffer* source, crux_buffer* batch) {
  const bool on = crux_sw().sac_tile_ops && !crux_sw().no_fused_epoch && !crux_sw().no_chained_epochs;
  const int64_t B = batch->capacity;
  if (!on || !net->has_adam) return false;
  if (source->prioritized && !crux_per_fused_gather()) return false;
  crux_mlp* both[2] = {net, tnet};
  for (crux_mlp* n : both) if (n->nd.L != 3 || !crux_dense_fwd_fused(n) || n->nd.acts[2] != CRUX_ACT_IDENTITY || n->nd.dims[2] != net->nd.dims[2] || n->nd.dims[3] != net->nd.dims[3] || n->nd.dims[0] != batch->obs_dim) return false;
  if (!crux_dense_bwd_fused3(net, B)) return false;
  return batch->act_kind == CRUX_ACTION_DISCRETE && batch->act_dim == net->nd.dims[3] && net->nd.dims[3] <= 4;
}
// One value_training call of the DQN family (see run_family). The target function is named, not inferred from alpha; DqnTdArgs::softq_alpha keeps its convention on the
// device (0 = dqn_target): device_alpha().
struct DqnRun {
  enum Target { TARGET_DQN, TARGET_SOFTQ };
  crux_mlp *net, *target_net; crux_buffer *source, *batch; float gamma; Target target; float alpha; int32_t use_weight; float beta; uint64_t sample_counter0; int32_t n_epochs;
  float polyak_tau;      // >= 0: polyak_average!(target_net, net, tau) behind the last epoch (tail)
  static constexpr int NROWS = 1; static constexpr bool ONE_READBACK = false; static constexpr const char *who = "dqn", *family = "DQN";
  float device_alpha() const { return target == TARGET_SOFTQ ? alpha : 0.f; }
  bool valid() const { return net && target_net && source && batch && n_epochs >= 1; }
  crux_ctx* ctx() const { return net->ctx; }      bool chain() const { return dqn_chain_case(net, target_net); }
  crux_buffer* per() const { return source->prioritized ? source : nullptr; }      unsigned rows(int) const { return 1u; }
  int shift(int) const { return chain() && dqn_tile_case(net, target_net, source, batch) ? -1 : 0; }      // tile plan: the info op writes the caller's row itself
  // polyak_average!(pi_minus, pi, tau) after the epoch loop (off_policy.jl:108: the DQN family updates its target once per value_training call) as an op of the chain: it needs
  // the last epoch's Adam (phase 5) and shares the launch of that epoch's info / beta-power phase -- the stand-alone PolyakOp launch (~5 us of a 230 us C3 iteration) is gone.
  int32_t tail() const { return polyak_tau >= 0.f ? crux_polyak(target_net, net, polyak_tau) : CRUX_OK; }
  int32_t epoch(int e, float* const* host_rows) const;
  int32_t epoch_tiles(uint64_t sample_counter, float* info_out, float* d_y, float* d_err) const;      // the chained C3 family
};
int32_t DqnRun::epoch_tiles(uint64_t sample_counter, float* info_out, float* d_y, float* d_err) const {      // (the tile plan other files call dqn_epoch_tiles)
  crux_mlp* const tnet = target_net; const float softq_alpha = device_alpha();
  crux_ctx* c = net->ctx; const int64_t B = batch->capacity; const bool per = source->prioritized; const int nout = net->nd.dims[3], K = net->nd.dims[2];
  int32_t rc;
  // Phases: 0 uniform ids | 1 search + gather / gather | 2 forward (both nets) | 3 td tile (+ update_priorities!) | 4 pullback || leaf re-sum -> root paths (LeafTouchOp) |
  // 5 norm || Adam (AdamSelfOp) | 6 info, beta-power advance. Chained: the sampling of epoch e + 1 runs beside the tail of epoch e -- ids beside 4, search + gather beside 5 (the
  // replay tree is complete after 4; the gather rewrites the batch rows the pullback read: not before 5), forward beside 6 (after Adam): FOUR launches per epoch.
  const bool touch_split = per && (B > 256 || source->per_full_dirty);      // (root paths as an op of their own in 5: the search then waits one launch longer)
  const int ov = touch_split ? 2 : 3;
  auto bail = [&](int32_t e) { crux_exec_abort(c); return e; };
  EpochTags tg(c, true, "dqn_epoch", ov, ov);
  if (use_weight && !has_col(batch, CRUX_COL_WEIGHT)) return bail(crux_fail(c, CRUX_EINVAL, "td_loss(weight=:weight): batch has no :weight column"));
  rc = per ? crux_per_sample(batch, source, B, nullptr, beta, sample_counter) : crux_uniform_sample(batch, source, B, nullptr, sample_counter); if (rc) return bail(rc);
  tg.tag([](int kid, int&) { return kid == OP_UNIFORM_IDS ? 0 : (kid == OP_PER_SAMPLE || kid == OP_GATHER_RING_ALL || kid == OP_RING_IDS || kid == OP_COPY_F32) ? 1 : kid == OP_PER_UPDATE ? 2 : -1; });
  Carve cv{(char*)crux_scratch(c, 4 * (size_t)B * (nout + 2) + 8192), 0}; if (!cv.p) return bail(crux_fail(c, CRUX_ENOMEM, "dqn_epoch: scratch"));
  float* dy = cv.take<float>((size_t)B * nout); float* term = cv.take<float>((size_t)B); float* qsel = cv.take<float>((size_t)B);
  Carve sv{(char*)crux_exec_small(c, 256 * 6), 0}; if (!sv.p) return bail(crux_fail(c, CRUX_ENOMEM, "dqn_epoch: executor region"));
  float* dinfo = sv.take<float>(CRUX_INFO_N); double* ssq = sv.take<double>(2 + SUMSQ_BLOCKS); int32_t* status = sv.take<int32_t>(1); int32_t* nanf = sv.take<int32_t>(2);
  rc = crux_exec_zero(c, dinfo, 256 * 6, c->stream); if (rc) return bail(rc);
  ExecRec* r = rec_of(c); float* const info_dst = r->info_row_override ? r->info_row_override : dinfo;      // asynchronous chains: the info op writes the caller's device row itself (round 6: one launch less behind the chain's last epoch)
  if (r->info_row_override) { rc = crux_exec_zero(c, r->info_row_override, sizeof(float) * CRUX_INFO_N, c->stream); if (rc) return bail(rc); }
  tg.only(1);
  const float* S = (const float*)batch->col[CRUX_COL_S]; const float* SP = (const float*)batch->col[CRUX_COL_SP];
  rc = crux_dense_forward12(net, S, B, c->stream); if (!rc) rc = crux_dense_forward12(tnet, SP, B, c->stream); if (rc) return bail(rc);
  tg.only(2);
  { DqnTdArgs a{}; auto l3 = [&](crux_mlp* n) { const NetDesc& nd = n->nd; return TileSet{n->p + nd.woff[2], n->p + nd.boff[2], crux_dense_act(n, 2), crux_dense_act(n, 3)}; };
    a.qt = l3(tnet); a.q = l3(net); a.r = (const float*)batch->col[CRUX_COL_R]; a.done = (const uint8_t*)batch->col[CRUX_COL_DONE]; a.a = (const uint8_t*)batch->col[CRUX_COL_A];
    a.w = use_weight ? (const float*)batch->col[CRUX_COL_WEIGHT] : nullptr; a.gamma = gamma; a.softq_alpha = softq_alpha; a.nout = nout; a.K = K; a.B = (int32_t)B;
    a.y = d_y; a.dy = dy; a.err = per ? d_err : nullptr; a.term = term; a.qsel = qsel;
    a.per = per ? 1 : 0; a.pr = source->priorities; a.pminmax = source->pminmax; a.ids = batch->d_indices; a.per_alpha = source->alpha;
    crux_exec_push<DqnTdTileOp>(c, (unsigned)((B + 15) / 16), a); }
  tg.only(3);
  Sumsq2Fix fx{};
  rc = crux_dense_backward(net, S, B, dy, 1.0f, true, nullptr, c->stream, &fx, 0, nanf); if (rc) return bail(rc);
  tg.only(4);
  if (per) { rc = crux_per_touched(source, batch->d_indices, B, false, (unsigned*)(nanf + 2)); if (rc) return bail(rc);      // leaves + root paths as one op beside the pullback (LeafTouchOp)
    tg.tag([](int kid, int&) { return (kid == OP_LEAF_TOUCH || kid == OP_LEAF_REFRESH) ? 4 : kid == OP_TREE_TOUCH ? 5 : -1; }); }
  // 5: the norm (for the info row) and, beside it, Adam gated on the producers' NaN flags (AdamSelfOp, sac.hip) | 6: info, beta-power advance
  CRUX_RUN(c, Sumsq2Op, SUMSQ_BLOCKS, 256, c->stream, net->g, (int64_t)net->nd.n_params, (float*)nullptr, (int64_t)0, ssq, fx);
  rc = adam_self(net, nanf, status, fx, 0); if (rc) return bail(rc);
  tg.tag([](int kid, int&) { return kid == OP_ADAM_ADVANCE_SELF ? 6 : 5; });
  crux_exec_push<TdInfo2Op>(c, 1u, (const float*)term, (const float*)qsel, (const double*)ssq, B, info_dst);
  tg.only(6);
  crux_exec_add_readback(c, info_out, dinfo, status, "td_loss");
  return tg.finish(7);
}

// One epoch of value_training for the DQN family (src/model_free/off_policy.jl:69-93 with dqn_target, rl/dqn.jl:4-6): rand!(batch, source; i) ->
// y = target(pi_minus, batch) -> [td_error -> update_priorities!(source, batch.indices, .)] -> train!(pi, td_loss). Networks at least
// CRUX_DENSE_MIN_WIDTH wide run the whole epoch as ONE fused launch; narrower ones take the same steps one call at a time.
int32_t DqnRun::epoch(int e, float* const* host_rows) const {
  if (!net || !target_net || !source || !batch) return CRUX_EINVAL;
  const uint64_t sample_counter = sample_counter0 + (uint64_t)e; float* info_out = info_row(host_rows, 0, e);
  crux_ctx* c = net->ctx; const int64_t B = batch->capacity;
  const bool per = source->prioritized;
  const bool fuse = net->nd.maxdim >= CRUX_DENSE_MIN_WIDTH && target_net->nd.maxdim >= CRUX_DENSE_MIN_WIDTH && !crux_sw().no_fused_epoch;
  int32_t rc;
  if (per) { rc = crux_per_prepare(source); if (rc) return rc; }
  rc = grow_epoch_tmp(c, 8 * (size_t)B + 512, B, "dqn_epoch"); if (rc) return rc;      // targets and td errors
  float* d_y = (float*)c->epoch_tmp; float* d_err = (float*)((char*)c->epoch_tmp + ((4 * (size_t)B + 255) / 256) * 256);
  if (fuse && c->rec && rec_of(c)->chain && crux_exec_recording(c) && dqn_tile_case(net, target_net, source, batch))      // chained epochs of the C3 family: the tile op (5 launches per epoch)
    return epoch_tiles(sample_counter, info_out, d_y, d_err);
  auto bail = [&](int32_t e) { if (fuse) crux_exec_abort(c); return e; };
  // Phase plan of the fused epoch (L = number of Dense layers): the target network's forward chain runs beside the online network's, the replay
  // bookkeeping beside the backward chain.    0 search | 1 gather, ring ids, zero-fill | 2+k forward layer k (both nets; + push! priorities of the batch)
  //   2+L dqn_target | 3+L td head | 4+L+j backward of layer L-1-j (weight + data gradient; + update_priorities!, leaf re-sum, root paths) | then norm, info, Adam
  // chained epochs (crux_dqn_epochs): the sampling of epoch e + 1 (phase 0: search / uniform ids, phase 1: gather, ring ids, fills) touches nothing that the last three
  // phases of epoch e (norm | info + Adam | beta-power advance) read or write -- the batch rows and the sampled ids were last read by the first-layer weight gradient and
  // the tree refresh one phase earlier -- so it runs BESIDE them: phases 0 and 1 of a later epoch are tagged as the previous epoch's last-but-two and last-but-one, and
  // its remaining phases close up by THREE: the first forward layer of epoch e + 1 shares a launch with the beta-power advance of epoch e (the last phase, which writes
  // the two powers only; Adam of epoch e + 1 reads them nine phases later). The replay chain (leaf refresh -> root paths -> search -> gather) then hides the optimizer
  // tail instead of following it: 13 phases, 10 launches per chained epoch.
  // The overlap is bounded by the replay tree: update_priorities! -> leaf re-sum -> root paths of epoch e sit at phases 4+L-sq .. 6+L-sq and read batch->d_indices / write
  // the tree total, which the search of epoch e + 1 (phase 4+2L-sq with the full overlap of three) rewrites and probes. With fewer than three Dense layers the backward
  // chain is too short to cover them, so the overlap shrinks to L phases there (search(e + 1) strictly after the root paths of e).
  // Round 4 (dense_fused.h): a network whose first two layers run as ONE forward launch (Fwd12Op) has nf = Ld - 1 forward launches, and one whose layer-1 / layer-0
  // pullback runs as one phase (Wgrad2Op || Dgrad2W1Op) nb = Ld - 1 backward phases; the plan below is written in nf, nb. With the sequential group (sq) the replay
  // chain starts INSIDE the head's block: update_priorities! is a second sequential tail behind the td head (one block, reads the head's td errors), so the leaf
  // re-sum and the root paths sit at 3 + nf and 4 + nf, and the search of epoch e + 1 (phase 7 + nf + nb - sq - ov of this epoch) stays behind the root paths as long
  // as ov <= nb + 1; without the group the chain is update | leaf | paths at 4 + nf - sq .., and ov <= nb as before.
  const NetPlan pn = net_plan(net, B); const bool ffw = crux_dense_fwd_fused(net);
  const int nf = pn.nf, nb = pn.nb;
  const int sq0 = B <= 256 ? 1 : 0;
  const bool tailp = per && sq0 == 1;
  // sph: with the search and the gather in one launch (PerSampleGatherOp) the sampling of an epoch is phase 1 alone, so the search of epoch e + 1 sits one phase later and the
  // overlap may be one deeper
  const int sph = (per && crux_per_fused_gather()) ? 1 : 0;
  const int ovmax = (tailp ? nb + 1 : nb) + sph;
  const int ov = per ? (ovmax < 1 ? 1 : (ovmax < 3 ? ovmax : 3)) : 3;
  // the target (one block at B <= 256) and the loss head (one block) are a sequential pair: the head runs in the target's block, right after it, and every later
  // phase moves up by one (sq).
  const int sq = sq0;
  if (fuse && !crux_exec_recording(c)) { rc = crux_exec_begin(c); if (rc) return bail(rc); }      // (a chained recording is already open)
  EpochTags tg(c, fuse, "dqn_epoch", ov, ov);
  if (crux_dense_fwd_fused(target_net) != ffw || target_net->nd.L != net->nd.L) tg.plan_ok = false;
  rc = per ? crux_per_sample(batch, source, B, nullptr, beta, sample_counter) : crux_uniform_sample(batch, source, B, nullptr, sample_counter); if (rc) return bail(rc);
  tg.tag([&](int kid, int&) { return (kid == OP_PER_SEARCH || kid == OP_UNIFORM_IDS) ? 0 : (kid == OP_PER_SAMPLE || kid == OP_GATHER_RING_ALL || kid == OP_RING_IDS || kid == OP_COPY_F32) ? 1 : kid == OP_PER_UPDATE ? 2 : -1; });
  rc = target == TARGET_SOFTQ ? crux_softq_target(target_net, batch, gamma, alpha, d_y) : crux_dqn_target(target_net, batch, gamma, d_y); if (rc) return bail(rc);      // softq_target(alpha) (rl/softq.jl:4-13) | dqn_target (rl/dqn.jl:4-6)
  tg.tag([&](int kid, int& g) { if (kid == OP_FWD12) { g = 1; return 2; }
    return kid == OP_GEMM ? (g < nf ? 2 + g++ : -1) : (kid == OP_DQN_TARGET || kid == OP_SOFTQ_TARGET) ? (2 + nf) | (sq ? PH_SEQ_HEAD : 0) : -1; });
  auto td_rule = [&](int kid, int& g) {      // g counts the GEMMs: Ld forward, then (weight, data) pairs from the last layer down, the first layer has no data gradient
    if (kid == OP_FILL) return 1;
    if (kid == OP_FWD12) { g = 1; return 2; }
    if (kid == OP_GEMM) { const int k = g++; if (k < nf) return 2 + k; const int j = pn.stage(k - nf); return j < nb ? 4 + nf + j - sq : -1; }
    if (kid == OP_WGRAD2 || kid == OP_DGRAD2W1) return 3 + nf + nb - sq;      // the last backward phase: layer 1's dW beside layer 1's dX -> layer 0's dW
    if (kid == OP_TD_HEAD) return sq ? ((2 + nf) | PH_SEQ_TAIL) : 3 + nf;
    if (kid == OP_SUMSQ2) return 4 + nf + nb - sq; if (kid == OP_TD_INFO || kid == OP_ADAM_GATED) return 5 + nf + nb - sq; if (kid == OP_ADAM_ADVANCE) return 6 + nf + nb - sq;
    return -1; };
  if (per) { rc = crux_td_step_with_error(net, batch, d_y, use_weight, d_err, info_out); if (rc) return bail(rc);
    tg.tag(td_rule);
    rc = crux_per_update_device(source, batch->d_indices, d_err, B); if (rc) return bail(rc);
    tg.tag([&](int kid, int&) { if (tailp) return kid == OP_PER_UPDATE ? ((2 + nf) | PH_SEQ_TAIL) : kid == OP_LEAF_REFRESH ? 3 + nf : kid == OP_TREE_TOUCH ? 4 + nf : -1;
      return kid == OP_PER_UPDATE ? 4 + nf - sq : kid == OP_LEAF_REFRESH ? 5 + nf - sq : kid == OP_TREE_TOUCH ? 6 + nf - sq : -1; }); }
  else { rc = crux_td_step(net, batch, d_y, use_weight, info_out); if (rc) return bail(rc); tg.tag(td_rule); }
  return tg.finish(7 + nf + nb - sq);
}

int32_t crux_dqn_epoch(crux_mlp* net, crux_mlp* target_net, crux_buffer* source, crux_buffer* batch, float gamma, int32_t use_weight, float beta,
                       uint64_t sample_counter, float* info_out) { CRUX_PLAIN_ONLY("crux_dqn_epoch", net, target_net); CRUX_NO_CLIP("crux_dqn_epoch", net);
  return DqnRun{net, target_net, source, batch, gamma, DqnRun::TARGET_DQN, 0.f, use_weight, beta, sample_counter, 1, -1.f}.epoch(0, &info_out);
}
// value_training's epoch loop (off_policy.jl:69: `for epoch in 1:c_opt.epochs`) for the DQN family as ONE recorded list: the n epochs are recorded back to back, the
// phases of epoch e follow those of epoch e - 1, and the host uploads, launches and reads back once. Epoch e draws with sample counter sample_counter0 + e; beta is
// the iteration's (rand!(…, i = S.i)). infos: host [n x CRUX_INFO_N]. Falls back to n single-epoch calls wherever an epoch cannot be chained (narrow networks, a
// priority tree that needs a full rebuild between epochs).
int32_t crux_dqn_epochs(crux_mlp* net, crux_mlp* target_net, crux_buffer* source, crux_buffer* batch, float gamma, int32_t use_weight, float beta,
                        uint64_t sample_counter0, int32_t n_epochs, float* infos) { CRUX_PLAIN_ONLY("crux_dqn_epochs", net, target_net); CRUX_NO_CLIP("crux_dqn_epochs", net);
  return run_family(DqnRun{net, target_net, source, batch, gamma, DqnRun::TARGET_DQN, 0.f, use_weight, beta, sample_counter0, n_epochs, -1.f}, &infos, nullptr);
}
// the same loop with softq_target(alpha) (rl/softq.jl:4-13) in place of dqn_target: SoftQ's value_training
int32_t crux_softq_epochs(crux_mlp* net, crux_mlp* target_net, crux_buffer* source, crux_buffer* batch, float gamma, float alpha, int32_t use_weight, float beta,
                          uint64_t sample_counter0, int32_t n_epochs, float* infos) { CRUX_PLAIN_ONLY("crux_softq_epochs", net, target_net); CRUX_NO_CLIP("crux_softq_epochs", net);
  if (!(alpha > 0.f)) return CRUX_EINVAL;
  return run_family(DqnRun{net, target_net, source, batch, gamma, DqnRun::TARGET_SOFTQ, alpha, use_weight, beta, sample_counter0, n_epochs, -1.f}, &infos, nullptr);
}
// value_training of the DQN family INCLUDING its target update (off_policy.jl:66-111 with :108) WITHOUT the host, for the iteration loop of solve(::OffPolicySolver): nothing
// is read back or waited for; the info row of epoch e lands in d_infos[e] (device, [n_epochs x CRUX_INFO_N]) when the device gets there (a NaN gradient norm shows there), and
// polyak_average!(target_net, net, tau) rides in the last epoch's final phase (tau < 0: none). softq_alpha == 0 selects dqn_target, > 0 softq_target(alpha): a SoftQ caller
// must pass alpha > 0. CRUX_EUNSUP for networks that do not take the recorded form (the caller uses crux_dqn_epochs / crux_softq_epochs).
int32_t crux_dqn_value_training_async(crux_mlp* net, crux_mlp* target_net, crux_buffer* source, crux_buffer* batch, float gamma, float softq_alpha, int32_t use_weight, float beta,
                                      uint64_t sample_counter0, int32_t n_epochs, float tau, float* d_infos) { CRUX_PLAIN_ONLY("crux_dqn_value_training_async", net, target_net); CRUX_NO_CLIP("crux_dqn_value_training_async", net);
  if (!d_infos || softq_alpha < 0.f || tau > 1.f) return CRUX_EINVAL;
  if (!net || !target_net || !dqn_chain_case(net, target_net)) return CRUX_EUNSUP;
  if (tau >= 0.f && net->nd.n_params != target_net->nd.n_params) return crux_fail(net->ctx, CRUX_EINVAL, "value_training: polyak_average! needs equal parameter counts");
  const DqnRun run{net, target_net, source, batch, gamma, softq_alpha > 0.f ? DqnRun::TARGET_SOFTQ : DqnRun::TARGET_DQN, softq_alpha, use_weight, beta, sample_counter0, n_epochs, tau};
  return run_family(run, nullptr, d_infos);
}

int32_t crux_sac_target(crux_mlp* actor, crux_mlp* q1t, crux_mlp* q2t, crux_mlp* la, crux_buffer* b, float gamma, uint64_t seed, uint64_t counter, float* d_y);
int32_t crux_sac_temp_step(crux_mlp* actor, crux_mlp* la, crux_buffer* b, float H_target, uint64_t seed, uint64_t counter, float* info_out);
int32_t crux_double_q_step(crux_mlp* q1, crux_mlp* q2, crux_buffer* b, const float* d_y, int32_t use_weight, float* info_out);
int32_t crux_sac_actor_step(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* la, crux_buffer* b, uint64_t seed, uint64_t counter, float* info_out);
int32_t crux_q_step(crux_mlp* q, crux_buffer* b, const float* d_y, int32_t use_weight, float* info_out);
int32_t crux_dpg_target(crux_mlp* actor_t, crux_mlp* q1t, crux_mlp* q2t, crux_buffer* b, float gamma, float sigma, float eps_min, float eps_max, float a_min, float a_max,
                        uint64_t seed, uint64_t counter, float* d_y);
int32_t crux_dpg_actor_step(crux_mlp* actor, crux_mlp* q, crux_buffer* b, float* info_out);

// The SAC epoch on the fused block kernels and the per-sample-tile ops of sac_fused.h (round 4): 17 phases, 14 launches per epoch inside a chain (round 3: 30 / 26).
//   0 ids | 1 gather, zero-fills | 2 actor(s') layers 0+1 ; vcat(s, a) | 3 actor(s') output layer + exploration -> (s', a'), log pi ; Q1, Q2 (s, a) layers 0+1
//   4 target Q1, Q2 (s', a') layers 0+1 ; actor(s) layers 0+1 | 5 the four critic output layers + sac_target + both double_Q_loss heads ; actor(s) output layer + the TWO
//   exploration draws of the temperature and the actor step (same means: the temperature step leaves the actor untouched) | 6 critic pullbacks (one phase each network) ;
//   temperature head | 7 norm ; Adam(log alpha) | 8 info, Adam(Q1), Adam(Q2) | 9 Q1, Q2 (s, a~) layers 0+1 | 10 their output layers + sac_actor_loss head
//   11 critic input gradients down to layer 0's dZ | 12 layer 0's W' dZ + reverse of exploration | 13 actor pullback ; logSigma row sums | 14 norm | 15 info, Adam | 16 advance, polyak
// The order inside every chain is the reference's (temperature, critic and actor each see what the previous step left; sac_target reads log alpha BEFORE the temperature
// update lands, the actor head after). Same arithmetic as the generic recording below (tools/fused_check.py compares the two bit for bit); false = not this case.
struct SacRun {      // one value_training call with SAC's pieces (crux_sac_epoch, crux_sac_epochs[_async]): see run_family
  crux_mlp *actor, *q1, *q2, *actor_targ, *q1_targ, *q2_targ, *log_alpha; crux_buffer *source, *batch; float gamma, H_target, tau; int32_t use_weight, epoch0, n_epochs, critic_every, actor_every;
  uint64_t sample_counter0, noise_seed, noise_counter0;
  static constexpr int NROWS = 3; static constexpr bool ONE_READBACK = true; static constexpr const char *who = "sac", *family = "SAC";
  bool valid() const { return actor && q1 && q2 && q1_targ && q2_targ && log_alpha && source && batch && n_epochs >= 1 && critic_every >= 1 && actor_every >= 1; }
  crux_ctx* ctx() const { return actor->ctx; }      crux_buffer* per() const { return nullptr; }      int32_t tail() const { return CRUX_OK; }
  bool chain() const { return !crux_sw().no_fused_epoch && !crux_sw().no_chained_epochs; }
  bool uc(int e) const { return (epoch0 + e) % critic_every == 0; }      bool ua(int e) const { return (epoch0 + e) % actor_every == 0; }
  // rows 3 e .. 3 e + 2: temperature, [critics], [actor]. Tile plans: the actor's info op sits IN the epoch's last phase -- the copies join the launch after it, the next epoch's third
  unsigned rows(int e) const { return 1u | (uc(e) ? 2u : 0u) | (ua(e) ? 4u : 0u); }
  int shift(int e) const { return tile_case(uc(e), ua(e)) ? 4 : 0; }
  int32_t epoch(int e, float* const* host_rows) const {
    return one(uc(e), ua(e), sample_counter0 + (uint64_t)e, noise_counter0 + 3ull * (uint64_t)e, info_row(host_rows, 0, e), info_row(host_rows, 1, e), info_row(host_rows, 2, e)); }
  int32_t one(int32_t update_critic, int32_t update_actor, uint64_t sample_counter, uint64_t noise_counter, float* info_temp, float* info_critic, float* info_actor) const;
  bool tile_case(int32_t uc, int32_t ua) const;
  int32_t epoch_tiles(uint64_t sample_counter, uint64_t noise_counter, float* info_temp, float* info_critic, float* info_actor) const;
};
bool SacRun::tile_case(int32_t uc, int32_t ua) const {
  crux_mlp* const q1t = q1_targ, * const q2t = q2_targ;
  const bool on = crux_sw().sac_tile_ops && !crux_sw().no_fused_epoch;      // (read per call: tests switch forms inside one process)
  if (!on || !uc || !ua || source->prioritized) return false;
  const int64_t B = batch->capacity; crux_mlp* all[5] = {actor, q1, q2, q1t, q2t};
  for (crux_mlp* n : all) { if (n->nd.L != 3 || !crux_dense_fwd_fused(n) || n->nd.acts[2] != CRUX_ACT_IDENTITY || n->nd.dims[2] != actor->nd.dims[2]) return false; }
  if (!crux_dense_bwd_fused3(actor, B) || !crux_dense_bwd_fused3(q1, B) || !crux_dense_bwd_fused3(q2, B)) return false;
  // (a two-headed actor stays off the tile plan, whose ops read constant logSigma extras: its 2 act_dim output rows already fail dims[3] == act_dim, and the flag says so by name)
  if (actor->sigma_head || batch->act_dim > 4 || batch->obs_dim + batch->act_dim > 16 || actor->nd.dims[3] != batch->act_dim || q1->nd.dims[3] != 1 || q2->nd.dims[3] != 1) return false;
  if (q1t->nd.dims[3] != 1 || q2t->nd.dims[3] != 1 || q1->nd.dims[0] != batch->obs_dim + batch->act_dim) return false;
  return true;
}
int32_t SacRun::epoch_tiles(uint64_t sample_counter, uint64_t noise_counter, float* info_temp, float* info_critic, float* info_actor) const {      // (the tile plan other files call sac_epoch_tiles)
  crux_mlp* const q1t = q1_targ, * const q2t = q2_targ, * const la = log_alpha;
  crux_ctx* c = actor->ctx; const int64_t B = batch->capacity; const int od = batch->obs_dim, ad = batch->act_dim, sd = od + ad, K = actor->nd.dims[2];
  int32_t rc = CRUX_OK;
  if (use_weight && !has_col(batch, CRUX_COL_WEIGHT)) return crux_fail(c, CRUX_EINVAL, "double_Q_loss(weight=:weight): batch has no :weight column");
  if (!crux_exec_recording(c)) { rc = crux_exec_begin(c); if (rc) return rc; }
  auto bail = [&](int32_t e) { crux_exec_abort(c); return e; };
  EpochTags tg(c, true, "sac_epoch", 3, 3);
  // buffers of this epoch (scratch of the recording: live until the list has run)
  float* y = (float*)crux_exec_small(c, 4 * (size_t)B); if (!y) return bail(crux_fail(c, CRUX_EUNSUP, "sac_epoch: batch of %lld rows exceeds the executor's region", (long long)B));
  Carve cv{(char*)crux_scratch(c, 4 * (size_t)B * (3 * sd + 3 * ad + 12) + 65536), 0}; if (!cv.p) return bail(crux_fail(c, CRUX_ENOMEM, "sac_epoch: scratch"));
  float* sa_c = cv.take<float>((size_t)B * sd); float* sa_t = cv.take<float>((size_t)B * sd); float* sa_a = cv.take<float>((size_t)B * sd);
  float* lp_t = cv.take<float>((size_t)B); float* lp_temp = cv.take<float>((size_t)B); float* lp_a = cv.take<float>((size_t)B); float* eps = cv.take<float>((size_t)B * ad);
  float* dy1 = cv.take<float>((size_t)B); float* dy2 = cv.take<float>((size_t)B); float* t1 = cv.take<float>((size_t)B); float* t2 = cv.take<float>((size_t)B);
  float* da1 = cv.take<float>((size_t)B); float* da2 = cv.take<float>((size_t)B); float* ta = cv.take<float>((size_t)B); float* dmu = cv.take<float>((size_t)B * ad); float* dls = cv.take<float>((size_t)B * ad);
  // info rows / statistics / status words of the three steps
  Carve st_{(char*)crux_exec_small(c, 256 * 5), 0}, sc_{(char*)crux_exec_small(c, 256 * 6), 0}, sa_{(char*)crux_exec_small(c, 256 * 6), 0};
  if (!st_.p || !sc_.p || !sa_.p) return bail(crux_fail(c, CRUX_ENOMEM, "sac_epoch: executor region"));
  float* it = st_.take<float>(CRUX_INFO_N); double* ssq_t = st_.take<double>(2 + SUMSQ_BLOCKS); int32_t* stt = st_.take<int32_t>(1);
  float* ic = sc_.take<float>(CRUX_INFO_N); double* ssq_c = sc_.take<double>(2 + SUMSQ_BLOCKS); int32_t* stc = sc_.take<int32_t>(1); int32_t* nfc = sc_.take<int32_t>(2);
  float* ia = sa_.take<float>(CRUX_INFO_N); double* ssq_a = sa_.take<double>(2 + SUMSQ_BLOCKS); int32_t* sta = sa_.take<int32_t>(1); int32_t* nfa = sa_.take<int32_t>(2);
  const float* S = (const float*)batch->col[CRUX_COL_S]; const float* SP = (const float*)batch->col[CRUX_COL_SP];
  const float* ls = actor->p + actor->nd.xoff; const float* w = use_weight ? (const float*)batch->col[CRUX_COL_WEIGHT] : nullptr;
  auto l3 = [&](crux_mlp* n, bool store) { const NetDesc& nd = n->nd; return TileSet{n->p + nd.woff[2], n->p + nd.boff[2], crux_dense_act(n, 2), store ? crux_dense_act(n, 3) : nullptr}; };
  const unsigned nt = (unsigned)((B + 15) / 16);
  // 0, 1: rand!
  rc = crux_uniform_sample(batch, source, B, nullptr, sample_counter); if (rc) return bail(rc);
  tg.tag([](int kid, int&) { return kid == OP_UNIFORM_IDS ? 0 : kid == OP_GATHER_RING_ALL ? 1 : -1; });
  rc = check_sac(c, actor, q1, q2, la, batch, "sac_epoch"); if (rc) return bail(rc);
  rc = crux_exec_zero(c, it, 256 * 5, c->stream); if (!rc) rc = crux_exec_zero(c, ic, 256 * 6, c->stream); if (!rc) rc = crux_exec_zero(c, ia, 256 * 6, c->stream);
  if (!rc) rc = crux_exec_zero(c, la->g, sizeof(float) * (size_t)la->nd.n_params, c->stream); if (rc) return bail(rc);
  tg.only(1);
  // 2
  rc = crux_dense_forward12(actor, SP, B, c->stream); if (rc) return bail(rc);
  CRUX_RUN(c, ConcatSaOp, nblk(B * sd), 256, c->stream, S, (const float*)batch->col[CRUX_COL_A], od, ad, B, sa_c);
  tg.only(2);
  // 3
  { ActorExploreArgs a{}; a.mu = l3(actor, true); a.ls = ls; a.s = SP; a.od = od; a.ad = ad; a.K = K; a.B = (int32_t)B; a.n_cfg = 1; a.seed = noise_seed; a.cfg[0] = ExploreCfg{noise_counter, sa_t, lp_t, nullptr};
    crux_exec_push<ActorExploreTileOp>(c, nt, a); }
  rc = crux_dense_forward12(q1, sa_c, B, c->stream); if (!rc) rc = crux_dense_forward12(q2, sa_c, B, c->stream); if (rc) return bail(rc);
  tg.only(3);
  // 4
  rc = crux_dense_forward12(q1t, sa_t, B, c->stream); if (!rc) rc = crux_dense_forward12(q2t, sa_t, B, c->stream); if (!rc) rc = crux_dense_forward12(actor, S, B, c->stream); if (rc) return bail(rc);
  tg.only(4);
  // 5
  { SacCriticArgs a{}; a.q1t = l3(q1t, true); a.q2t = l3(q2t, true); a.q1 = l3(q1, true); a.q2 = l3(q2, true); a.r = (const float*)batch->col[CRUX_COL_R]; a.done = (const uint8_t*)batch->col[CRUX_COL_DONE];
    a.lp = lp_t; a.log_alpha = la->p; a.w = w; a.gamma = gamma; a.scale = 0.5f; a.K = K; a.B = (int32_t)B; a.y = y; a.dy1 = dy1; a.dy2 = dy2; a.term1 = t1; a.term2 = t2;
    crux_exec_push<SacCriticTileOp>(c, nt, a); }
  { ActorExploreArgs a{}; a.mu = l3(actor, true); a.ls = ls; a.s = S; a.od = od; a.ad = ad; a.K = K; a.B = (int32_t)B; a.n_cfg = 1; a.seed = noise_seed;      // the two draws side by side (each re-evaluates the output layer: 8 MFMAs)
    a.cfg[0] = ExploreCfg{noise_counter + 1, nullptr, lp_temp, nullptr}; crux_exec_push<ActorExploreTileOp>(c, nt, a);
    a.cfg[0] = ExploreCfg{noise_counter + 2, sa_a, lp_a, eps}; crux_exec_push<ActorExploreTileOp>(c, nt, a); }
  tg.only(5);
  // 6
  Sumsq2Fix fxc{}, fxa{};
  rc = crux_dense_backward(q1, sa_c, B, dy1, 1.0f, true, nullptr, c->stream, &fxc, 0, nfc); if (!rc) rc = crux_dense_backward(q2, sa_c, B, dy2, 1.0f, true, nullptr, c->stream, &fxc, 1, nfc); if (rc) return bail(rc);
  CRUX_RUN(c, TempHeadOp, 1, 256, c->stream, (const float*)lp_temp, B, H_target, (const float*)la->p, la->g, it, ssq_t);
  tg.only(6);
  // 7: the critics' norm (for the info row) and, beside it, their Adam steps gated on the pullback's NaN flags (AdamSelfOp, sac.hip); log alpha's step (+ 8: the advances)
  CRUX_RUN(c, Sumsq2Op, SUMSQ_BLOCKS, 256, c->stream, q1->g, (int64_t)q1->nd.n_params, q2->g, (int64_t)q2->nd.n_params, ssq_c, fxc);
  rc = adam_self(q1, nfc, stc, fxc, 0); if (!rc) rc = adam_self(q2, nfc, stc, fxc, 1); if (!rc) rc = adam_gated(la, ssq_t, stt, false); if (rc) return bail(rc);
  tg.tag([](int kid, int&) { return (kid == OP_ADAM_ADVANCE || kid == OP_ADAM_ADVANCE_SELF) ? 8 : 7; });
  // 8: critic info | the updated critics' first two layers on (s, a ~ pi)
  crux_exec_push<CriticInfo2Op>(c, 1u, (const float*)t1, (const float*)crux_dense_act(q1, 3), (const float*)t2, (const float*)crux_dense_act(q2, 3), (const double*)ssq_c, B, ic);
  rc = crux_dense_forward12(q1, sa_a, B, c->stream); if (!rc) rc = crux_dense_forward12(q2, sa_a, B, c->stream); if (rc) return bail(rc);
  tg.only(8);
  // 9
  { SacActorArgs a{}; a.q1 = l3(q1, true); a.q2 = l3(q2, true); a.lp = lp_a; a.log_alpha = la->p; a.K = K; a.B = (int32_t)B; a.dy1 = da1; a.dy2 = da2; a.term = ta;
    crux_exec_push<SacActorTileOp>(c, nt, a); }
  tg.only(9);
  // 10
  const float* dz1a = nullptr; const float* dz1b = nullptr;
  rc = crux_dense_dgrad_to_dz1(q1, sa_a, B, da1, &dz1a, c->stream); if (!rc) rc = crux_dense_dgrad_to_dz1(q2, sa_a, B, da2, &dz1b, c->stream); if (rc) return bail(rc);
  tg.only(10);
  // 11
  { CriticDxArgs a{}; a.c1 = TileSet{q1->p + q1->nd.woff[0], nullptr, dz1a, nullptr}; a.c2 = TileSet{q2->p + q2->nd.woff[0], nullptr, dz1b, nullptr};
    a.sa = sa_a; a.mu = crux_dense_act(actor, 3); a.eps = eps; a.ls = ls; a.log_alpha = la->p; a.od = od; a.ad = ad; a.K = q1->nd.dims[1]; a.B = (int32_t)B; a.dmu = dmu; a.dls = dls;
    crux_exec_push<CriticDxActorGradTileOp>(c, nt, a); }
  tg.only(11);
  // 12
  rc = crux_dense_backward(actor, S, B, dmu, 1.0f, true, nullptr, c->stream, &fxa, 0, nfa); if (rc) return bail(rc);
  CRUX_RUN(c, RowsumOp, ad, 256, c->stream, (const float*)dls, ad, B, actor->g + actor->nd.xoff, nfa);
  tg.only(12);
  // 13: the actor's norm | its Adam step (self-gated)
  CRUX_RUN(c, Sumsq2Op, SUMSQ_BLOCKS, 256, c->stream, actor->g, (int64_t)actor->nd.n_params, (float*)nullptr, (int64_t)0, ssq_a, fxa);
  rc = adam_self(actor, nfa, sta, fxa, 0); if (rc) return bail(rc);
  tg.tag([](int kid, int&) { return kid == OP_ADAM_ADVANCE_SELF ? 14 : 13; });
  // 14: actor info, polyak
  crux_exec_push<ActorInfo2Op>(c, 1u, (const float*)ta, (const float*)lp_a, (const double*)ssq_a, B, ia);
  if (actor_targ) { rc = crux_polyak(actor_targ, actor, tau); if (rc) return bail(rc); }
  rc = crux_polyak(q1t, q1, tau); if (!rc) rc = crux_polyak(q2t, q2, tau); if (rc) return bail(rc);
  tg.only(14);
  // the steps' read-backs in the order they ran (temperature, critics, actor), as the generic recording registers them
  crux_exec_add_readback(c, info_temp, it, stt, "sac_temp_loss"); crux_exec_add_readback(c, info_critic, ic, stc, "double_Q_loss"); crux_exec_add_readback(c, info_actor, ia, sta, "sac_actor_loss");
  // phases 0 / 1 of a chained epoch (ids | gather, fills) overlap the previous epoch's actor pullback (12: the gather rewrites the batch rows it read -- not before 13) and
  // norm + Adam (13), phase 2 (the new actor's forward on s') its info + advance + polyak (14): base + p - 3 for every p. 15 phases, 12 launches per chained epoch.
  return tg.finish(15);
}

// One epoch of value_training with SAC's pieces (off_policy.jl:69-104, rl/sac.jl): rand! -> sac_target -> train!(log_alpha, sac_temp_loss) ->
// [train!(critic, double_Q_loss)] -> [train!(actor, sac_actor_loss) -> polyak_average!(pi_minus, pi, tau)] as ONE fused launch.
int32_t SacRun::one(int32_t update_critic, int32_t update_actor, uint64_t sample_counter, uint64_t noise_counter, float* info_temp, float* info_critic, float* info_actor) const {
  if (!actor || !q1 || !q2 || !q1_targ || !q2_targ || !log_alpha || !source || !batch) return CRUX_EINVAL;
  crux_ctx* c = actor->ctx; const int64_t B = batch->capacity;
  if (source->prioritized) return crux_fail(c, CRUX_EUNSUP, "sac_epoch: prioritized replay over a DoubleNetwork critic is not defined (td_error, src/utils.jl:112)");
  if (c->rec && rec_of(c)->chain && tile_case(update_critic, update_actor))      // chained epochs of the C4 family: the tile ops (14 launches per epoch)
    return epoch_tiles(sample_counter, noise_counter, info_temp, info_critic, info_actor);
  const bool fuse = !crux_sw().no_fused_epoch;
  int32_t rc; float* d_y = nullptr;
  if (fuse) { if (!crux_exec_recording(c)) { rc = crux_exec_begin(c); if (rc) return rc; }       // a chained recording (crux_sac_epochs) is already open
    d_y = (float*)crux_exec_small(c, 4 * (size_t)B);
    if (!d_y) { crux_exec_abort(c); return crux_fail(c, CRUX_EUNSUP, "sac_epoch: batch of %lld rows exceeds the executor's region", (long long)B); } }
  else { rc = grow_epoch_tmp(c, 4 * (size_t)B + 256, B, "sac_epoch"); if (rc) return rc; d_y = (float*)c->epoch_tmp; }
  auto bail = [&](int32_t e) { if (fuse) crux_exec_abort(c); return e; };
  // Phase plan (LA = layers of the actor, LQ = of a critic; X = 3 + LA + LQ, Y = X + 4 + LQ). Chains that touch different networks run side by side:
  //   0 ids | 1 gather, zero-fills | 2.. actor(sp) forward ; vcat(s, a) ; Q1 || Q2 forward on (s, a) | 2+LA exploration at sp | 3+LA.. target Q1 || Q2 ; actor(s) forward
  //   X sac_target ; exploration at s | X+1 critic heads ; temperature head | X+2.. critic backward (weight || data gradient, both critics) ; Adam(log_alpha) | .. norm | info, Adam(Q1), Adam(Q2)
  //   X+1.. actor(s) forward of the ACTOR step, exploration (beside the critic's backward) | Y.. Q1 || Q2 forward | actor head | Q1 || Q2 input gradients | reverse of exploration | actor backward ; logSigma row sums | norm | info, Adam | polyak
  // The order inside every chain is the reference's (temperature before critic before actor: each sees the parameters the previous step left).
  // The temperature chain (X .. X + 3) is independent of the sequential group at X (ActorCriticPlan: the constants and the rules shared with DDPG / TD3).
  const ActorCriticPlan P(actor, q1, B, update_critic); const NetPlan& pa = P.pa; const int FA = P.FA, FQ = P.FQ, BA = P.BA, DQ = P.DQ, X = P.X, Y = P.Y;
  // a two-headed actor (crux_mlp_set_sigma_head) records SigmaExploreOp / SigmaActorGradOp where GaussExploreOp / ActorGradOp stand, in their phases; nothing takes
  // RowsumOp's place (the seed [dmu; dlogSigma] goes straight into the actor's pullback)
  const int EXPL = actor->sigma_head ? OP_SIGMA_EXPLORE : OP_GAUSS_EXPLORE, AGRAD = actor->sigma_head ? OP_SIGMA_ACTOR_GRAD : OP_ACTOR_GRAD;
  EpochTags tg(c, fuse, "sac_epoch", 3, 3);
  if (!P.ok(q2, q1_targ, q2_targ) || net_plan(q2, B).one != P.pq.one) tg.plan_ok = false;       // (the early actor forward needs X + 1 + FA < Y)
  // chained epochs: phases 0 (ids) and 1 (gather, fills) of a later epoch run beside the previous epoch's actor norm and info + Adam (neither reads the batch), and its
  // phase 2 (actor(sp) forward, vcat(s, a): online networks only) beside the previous epoch's advance + polyak, which writes beta powers and TARGET networks: the rest
  // closes up by three -- see crux_dqn_epoch
  rc = crux_uniform_sample(batch, source, B, nullptr, sample_counter); if (rc) return bail(rc);
  tg.tag([&](int kid, int&) { return P.sampling(kid); });
  rc = crux_sac_target(actor, q1_targ, q2_targ, log_alpha, batch, gamma, noise_seed, noise_counter, d_y); if (rc) return bail(rc);
  tg.tag([&](int kid, int& g) { return P.target(kid, g, EXPL, OP_SAC_TARGET); });
  rc = crux_sac_temp_step(actor, log_alpha, batch, H_target, noise_seed, noise_counter + 1, info_temp); if (rc) return bail(rc);
  tg.tag([&](int kid, int& g) { if (kid == OP_FILL) return 1; if (is_mm(kid)) { const int k = g++; return k < FA ? 3 + FA + k : -1; }
    return kid == EXPL ? X : kid == OP_TEMP_HEAD ? X + 1 : kid == OP_ADAM_GATED ? X + 2 : kid == OP_ADAM_ADVANCE ? X + 3 : -1; });
  if (update_critic) {
    rc = crux_double_q_step(q1, q2, batch, d_y, use_weight, info_critic); if (rc) return bail(rc);
    tg.tag([&](int kid, int& g) { return P.critic(kid, g); });
  }
  if (update_actor) {
    rc = crux_sac_actor_step(actor, q1, q2, log_alpha, batch, noise_seed, noise_counter + 2, info_actor); if (rc) return bail(rc);
    tg.tag([&](int kid, int& g) {      // GEMMs: LA actor forward, LQ + LQ critic forwards, LQ + LQ critic input gradients, then the actor's (weight, data) pairs
      if (kid == OP_FILL) return 1;
      // the actor's own forward pass and its exploration draw depend on neither the critic update nor the temperature: they run beside the critic's head / backward
      // phases (X + 1 ..), after the temperature step's last read of the actor's activations (its exploration at X)
      if (is_mm(kid)) { const int k = g++; if (k < FA) return X + 1 + k; if (k < FA + 2 * FQ) return Y + (k - FA) % FQ;
        if (k < FA + 2 * FQ + 2 * DQ) return Y + 1 + FQ + (k - FA - 2 * FQ) % DQ; return Y + 2 + FQ + DQ + pa.stage(k - FA - 2 * FQ - 2 * DQ); }
      return kid == EXPL ? X + 1 + FA : kid == OP_ACTOR_HEAD ? Y + FQ : kid == AGRAD ? Y + 1 + FQ + DQ : kid == OP_ROWSUM ? Y + 2 + FQ + DQ :
             kid == OP_SUMSQ2 ? Y + BA + 2 + FQ + DQ : (kid == OP_ACTOR_INFO || kid == OP_ADAM_GATED) ? Y + BA + 3 + FQ + DQ : kid == OP_ADAM_ADVANCE ? Y + BA + 4 + FQ + DQ : -1; });
    if (actor_targ) { rc = crux_polyak(actor_targ, actor, tau); if (rc) return bail(rc); }
    rc = crux_polyak(q1_targ, q1, tau); if (rc) return bail(rc);
    rc = crux_polyak(q2_targ, q2, tau); if (rc) return bail(rc);
    tg.tag([&](int kid, int&) { return kid == OP_POLYAK ? Y + BA + 4 + FQ + DQ : -1; });
  }
  return tg.finish(Y + BA + 5 + FQ + DQ);
}

int32_t crux_sac_epoch(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_mlp* log_alpha,
                       crux_buffer* source, crux_buffer* batch, float gamma, float H_target, float tau, int32_t use_weight, int32_t update_critic, int32_t update_actor,
                       uint64_t sample_counter, uint64_t noise_seed, uint64_t noise_counter0, float* info_temp, float* info_critic, float* info_actor) { CRUX_PLAIN_ONLY("crux_sac_epoch", actor, q1, q2, actor_targ, q1_targ, q2_targ, log_alpha); CRUX_NO_CLIP("crux_sac_epoch", actor, q1, q2, log_alpha);
  const SacRun run{actor, q1, q2, actor_targ, q1_targ, q2_targ, log_alpha, source, batch, gamma, H_target, tau, use_weight, 0, 1, 1, 1, sample_counter, noise_seed, noise_counter0};
  return run.one(update_critic, update_actor, sample_counter, noise_counter0, info_temp, info_critic, info_actor);
}
// value_training's epoch loop with SAC's pieces (off_policy.jl:69-104; SAC's c_opt.epochs = dN = 50, rl/sac.jl) in chains of up to 8 epochs per recorded list.
// Epoch e (global index epoch0 + e within the iteration) trains the critic when (epoch0 + e) % critic_every == 0 and the actor (then the target update) when
// (epoch0 + e) % actor_every == 0 (:91,96); it draws with sample counter sample_counter0 + e and noise counters noise_counter0 + 3 e .. + 2. infos_*: host [n x CRUX_INFO_N].
int32_t crux_sac_epochs(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_mlp* log_alpha,
                        crux_buffer* source, crux_buffer* batch, float gamma, float H_target, float tau, int32_t use_weight, int32_t epoch0, int32_t n_epochs,
                        int32_t critic_every, int32_t actor_every, uint64_t sample_counter0, uint64_t noise_seed, uint64_t noise_counter0,
                        float* infos_temp, float* infos_critic, float* infos_actor) { CRUX_PLAIN_ONLY("crux_sac_epochs", actor, q1, q2, actor_targ, q1_targ, q2_targ, log_alpha); CRUX_NO_CLIP("crux_sac_epochs", actor, q1, q2, log_alpha);
  float* const host_rows[3] = {infos_temp, infos_critic, infos_actor};
  return run_family(SacRun{actor, q1, q2, actor_targ, q1_targ, q2_targ, log_alpha, source, batch, gamma, H_target, tau, use_weight, epoch0, n_epochs, critic_every, actor_every,
                           sample_counter0, noise_seed, noise_counter0}, host_rows, nullptr);
}
// crux_sac_epochs without the host in the loop (see crux_dqn_value_training_async): d_infos is DEVICE memory, [n_epochs][3][CRUX_INFO_N] = temperature | critics | actor rows of every
// epoch (rows of steps an epoch skipped -- critic_every / actor_every -- are left as they were).
int32_t crux_sac_epochs_async(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_mlp* log_alpha,
                              crux_buffer* source, crux_buffer* batch, float gamma, float H_target, float tau, int32_t use_weight, int32_t epoch0, int32_t n_epochs,
                              int32_t critic_every, int32_t actor_every, uint64_t sample_counter0, uint64_t noise_seed, uint64_t noise_counter0, float* d_infos) { CRUX_PLAIN_ONLY("crux_sac_epochs_async", actor, q1, q2, actor_targ, q1_targ, q2_targ, log_alpha); CRUX_NO_CLIP("crux_sac_epochs_async", actor, q1, q2, log_alpha);
  if (!d_infos) return CRUX_EINVAL;
  return run_family(SacRun{actor, q1, q2, actor_targ, q1_targ, q2_targ, log_alpha, source, batch, gamma, H_target, tau, use_weight, epoch0, n_epochs, critic_every, actor_every,
                           sample_counter0, noise_seed, noise_counter0}, nullptr, d_infos);
}

// One epoch of value_training with DDPG's / TD3's pieces (off_policy.jl:69-104; rl/ddpg.jl, rl/td3.jl): rand! -> ddpg_target | td3_target -> [train!(critic, td_loss |
// double_Q_loss)] -> [train!(actor, -mean(Q(s, mu(s)))) -> polyak_average!] recorded as one list. q2 / q2_targ = NULL: single critic (DDPG); q2 with q2_targ = NULL:
// twin critics trained against a single-target (not used by the reference's solvers).
struct DpgRun {      // one value_training call with DDPG's / TD3's pieces (crux_dpg_epochs[_async]): see run_family
  crux_mlp *actor, *q1, *q2, *actor_targ, *q1_targ, *q2_targ; crux_buffer *source, *batch; float gamma, tau, sigma, eps_min, eps_max, a_min, a_max; int32_t use_weight, epoch0, n_epochs, critic_every, actor_every;
  uint64_t sample_counter0, noise_seed, noise_counter0;
  static constexpr int NROWS = 2; static constexpr bool ONE_READBACK = true; static constexpr const char *who = "dpg", *family = "DDPG / TD3";
  bool valid() const { return actor && q1 && actor_targ && q1_targ && source && batch && n_epochs >= 1 && critic_every >= 1 && actor_every >= 1; }
  crux_ctx* ctx() const { return actor->ctx; }      crux_buffer* per() const { return nullptr; }      int32_t tail() const { return CRUX_OK; }
  bool chain() const { return !crux_sw().no_chained_epochs; }
  bool uc(int e) const { return (epoch0 + e) % critic_every == 0; }      bool ua(int e) const { return (epoch0 + e) % actor_every == 0; }
  unsigned rows(int e) const { return (uc(e) ? 1u : 0u) | (ua(e) ? 2u : 0u); }      int shift(int) const { return 0; }      // rows 2 e (critic) and 2 e + 1 (actor)
  int32_t epoch(int e, float* const* host_rows) const { return one(uc(e), ua(e), sample_counter0 + (uint64_t)e, noise_counter0 + (uint64_t)e, info_row(host_rows, 0, e), info_row(host_rows, 1, e)); }
  int32_t one(int32_t update_critic, int32_t update_actor, uint64_t sample_counter, uint64_t noise_counter, float* info_critic, float* info_actor) const;
};
int32_t DpgRun::one(int32_t update_critic, int32_t update_actor, uint64_t sample_counter, uint64_t noise_counter, float* info_critic, float* info_actor) const {
  crux_ctx* c = actor->ctx; const int64_t B = batch->capacity;
  if (source->prioritized) return crux_fail(c, CRUX_EUNSUP, "dpg_epoch: DDPG / TD3 with a prioritized buffer is not wired up");
  int32_t rc;
  if (!crux_exec_recording(c)) { rc = crux_exec_begin(c); if (rc) return rc; }
  float* d_y = (float*)crux_exec_small(c, 4 * (size_t)B);
  if (!d_y) { crux_exec_abort(c); return crux_fail(c, CRUX_EUNSUP, "dpg_epoch: batch of %lld rows exceeds the executor's region", (long long)B); }
  auto bail = [&](int32_t e) { crux_exec_abort(c); return e; };
  // Phase plan (LA = layers of the actor, LQ = of a critic; X = 3 + LA + LQ, Y = X + 4 + LQ), chains that touch different networks side by side:
  //   0 ids | 1 gather, fills | 2.. target actor(sp) forward ; vcat(s, a) ; actor(s) forward of the ACTOR step | 2+LA target action (+ smoothing noise) ; mu(s) -> vcat(s, mu(s))
  //   3+LA.. target Q1 || Q2 forward (and, from 3: Q1 || Q2 forward on (s, a)) | X target | X+1 critic heads | X+2.. critic backward | norm | info, Adam | advance
  //   Y.. Q(s, mu(s)) forward | its input gradient | slice | actor backward | norm | info, Adam | advance, polyak
  const ActorCriticPlan P(actor, q1, B, update_critic); const NetPlan& pa = P.pa; const int LA = P.LA, FA = P.FA, FQ = P.FQ, BA = P.BA, DQ = P.DQ, Y = P.Y;
  // chained epochs: the sampling of epoch e + 1 beside the actor's norm and info + Adam of epoch e; its phase 2 reads the TARGET actor, which polyak (last phase) writes,
  // so the rest closes up by two only
  EpochTags tg(c, true, "dpg_epoch", 3, 2);
  const int ag = actor->nd.acts[LA - 1] != CRUX_ACT_IDENTITY ? 1 : 0;
  if (!P.ok(q2, q1_targ, q2_targ) || actor_targ->nd.L != LA || net_plan(actor_targ, B).nf != FA) tg.plan_ok = false;
  rc = crux_uniform_sample(batch, source, B, nullptr, sample_counter); if (rc) return bail(rc);
  tg.tag([&](int kid, int&) { return P.sampling(kid); });
  rc = crux_dpg_target(actor_targ, q1_targ, q2_targ, batch, gamma, sigma, eps_min, eps_max, a_min, a_max, noise_seed, noise_counter, d_y); if (rc) return bail(rc);
  tg.tag([&](int kid, int& g) { return P.target(kid, g, OP_DPG_ACTION, OP_DPG_TARGET); });
  if (update_critic) {
    rc = q2 ? crux_double_q_step(q1, q2, batch, d_y, use_weight, info_critic) : crux_q_step(q1, batch, d_y, use_weight, info_critic); if (rc) return bail(rc);
    tg.tag([&](int kid, int& g) { return P.critic(kid, g); });
  }
  if (update_actor) {
    rc = crux_dpg_actor_step(actor, q1, batch, info_actor); if (rc) return bail(rc);
    tg.tag([&](int kid, int& g) {      // GEMMs: LA actor forward, LQ critic forward, LQ critic input gradients, then the actor's (weight, data) pairs
      if (kid == OP_FILL) return 1;      // the info / status rows and the constant dQ = -1 / B
      if (is_mm(kid)) { const int k = g++; if (k < FA) return 2 + k; if (k < FA + FQ) return Y + (k - FA); if (k < FA + FQ + DQ) return Y + FQ + (k - FA - FQ);
        return Y + FQ + DQ + 1 + ag + pa.stage(k - FA - FQ - DQ); }
      if (kid == OP_ACT_GRAD) return ag ? Y + FQ + DQ + 1 : -1;      // dZ = act'(mu) .* dmu of a bounded (tanh) action head, between the slice and the actor's backward GEMMs
      return kid == OP_DPG_ACTION ? 2 + FA : kid == OP_SLICE_ROWS ? Y + FQ + DQ : kid == OP_SUMSQ2 ? Y + FQ + DQ + 1 + ag + BA : (kid == OP_MEAN_INFO || kid == OP_ADAM_GATED) ? Y + FQ + DQ + 2 + ag + BA :
             kid == OP_ADAM_ADVANCE ? Y + FQ + DQ + 3 + ag + BA : -1; });
    rc = crux_polyak(actor_targ, actor, tau); if (rc) return bail(rc);
    rc = crux_polyak(q1_targ, q1, tau); if (rc) return bail(rc);
    if (q2 && q2_targ) { rc = crux_polyak(q2_targ, q2, tau); if (rc) return bail(rc); }
    tg.tag([&](int kid, int&) { return kid == OP_POLYAK ? Y + FQ + DQ + 3 + ag + BA : -1; });
  }
  return tg.finish(Y + FQ + DQ + 4 + ag + BA);
}

// value_training's epoch loop with DDPG's / TD3's pieces in chains of up to 8 epochs per recorded list (see crux_sac_epochs). sigma < 0: no target-policy smoothing
// (DDPG); otherwise TD3's clamp(a' + clamp(sigma randn, eps_min, eps_max), a_min, a_max) with noise counters noise_counter0 + e. infos_*: host [n x CRUX_INFO_N].
int32_t crux_dpg_epochs(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_buffer* source, crux_buffer* batch,
                        float gamma, float tau, float sigma, float eps_min, float eps_max, float a_min, float a_max, int32_t use_weight, int32_t epoch0, int32_t n_epochs,
                        int32_t critic_every, int32_t actor_every, uint64_t sample_counter0, uint64_t noise_seed, uint64_t noise_counter0, float* infos_critic, float* infos_actor) { CRUX_PLAIN_ONLY("crux_dpg_epochs", actor, q1, q2, actor_targ, q1_targ, q2_targ); CRUX_NO_CLIP("crux_dpg_epochs", actor, q1, q2);
  float* const host_rows[2] = {infos_critic, infos_actor};
  return run_family(DpgRun{actor, q1, q2, actor_targ, q1_targ, q2_targ, source, batch, gamma, tau, sigma, eps_min, eps_max, a_min, a_max, use_weight, epoch0, n_epochs, critic_every, actor_every,
                           sample_counter0, noise_seed, noise_counter0}, host_rows, nullptr);
}
// crux_dpg_epochs without the host in the loop (see crux_dqn_value_training_async): d_infos is DEVICE memory, [n_epochs][2][CRUX_INFO_N] = critic | actor rows of every epoch
int32_t crux_dpg_epochs_async(crux_mlp* actor, crux_mlp* q1, crux_mlp* q2, crux_mlp* actor_targ, crux_mlp* q1_targ, crux_mlp* q2_targ, crux_buffer* source, crux_buffer* batch,
                              float gamma, float tau, float sigma, float eps_min, float eps_max, float a_min, float a_max, int32_t use_weight, int32_t epoch0, int32_t n_epochs,
                              int32_t critic_every, int32_t actor_every, uint64_t sample_counter0, uint64_t noise_seed, uint64_t noise_counter0, float* d_infos) { CRUX_PLAIN_ONLY("crux_dpg_epochs_async", actor, q1, q2, actor_targ, q1_targ, q2_targ); CRUX_NO_CLIP("crux_dpg_epochs_async", actor, q1, q2);
  if (!d_infos) return CRUX_EINVAL;
  return run_family(DpgRun{actor, q1, q2, actor_targ, q1_targ, q2_targ, source, batch, gamma, tau, sigma, eps_min, eps_max, a_min, a_max, use_weight, epoch0, n_epochs, critic_every, actor_every,
                           sample_counter0, noise_seed, noise_counter0}, nullptr, d_infos);
}
}  // extern "C"

// test hook: value(pi, x) through the executor (the same tile bodies as crux_mlp_forward_cached, run by the phase kernels) -- tests compare the two bit for bit
extern "C" int32_t crux_debug_exec_forward(crux_mlp* net, const float* d_x, int64_t B, float* d_y, int32_t with_backward, const float* d_dy) { CRUX_PLAIN_ONLY("crux_debug_exec_forward", net);
  if (!net || !d_x || !d_y) return CRUX_EINVAL;
  crux_ctx* c = net->ctx; int32_t rc = crux_exec_begin(c); if (rc) return rc;
  rc = crux_dense_forward(net, d_x, B, c->stream); if (rc) { crux_exec_abort(c); return rc; }
  if (with_backward) { rc = crux_dense_backward(net, d_x, B, d_dy, 1.0f, true, nullptr, c->stream); if (rc) { crux_exec_abort(c); return rc; } }
  rc = crux_exec_run(c); if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(d_y, crux_dense_act(net, net->nd.L), sizeof(float) * (size_t)net->nd.dims[net->nd.L] * (size_t)B, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CRUX_OK;
}

// test hook: n dependent trivial ops (a 256-float fill each): the executor's per-op overhead (dispatch + barrier)
extern "C" int32_t crux_debug_exec_nops(crux_ctx* c, int32_t n, int32_t blocks) {
  int32_t rc = crux_exec_begin(c); if (rc) return rc;
  float* p = (float*)crux_exec_small(c, 4 * 256 * (size_t)(blocks > 0 ? blocks : 1));
  for (int k = 0; k < n; ++k) crux_exec_push<FillOp>(c, (unsigned)(blocks > 0 ? blocks : 1), p, (float)k, (int64_t)256 * (blocks > 0 ? blocks : 1));
  return crux_exec_run(c);
}
// test hook: the forward pass of `net` recorded `reps` times (dependent ops): per-op cost of the tile GEMM inside the executor
extern "C" int32_t crux_debug_exec_forward_reps(crux_mlp* net, const float* d_x, int64_t B, int32_t reps) { CRUX_PLAIN_ONLY("crux_debug_exec_forward_reps", net);
  crux_ctx* c = net->ctx; int32_t rc = crux_exec_begin(c); if (rc) return rc;
  for (int k = 0; k < reps; ++k) { rc = crux_dense_forward(net, d_x, B, c->stream); if (rc) { crux_exec_abort(c); return rc; } }
  return crux_exec_run(c);
}
