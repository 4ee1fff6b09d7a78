"""The multi-GPU exchange step on ONE GPU: two contexts on device 0, wired into a replica group of two (crux_peer_attach_local), run the persistent
learner kernels concurrently; every minibatch step SUM-all-reduces the local gradients through the peer-slot protocol of train_mfma_kernel.h (the same
code path N processes on N GPUs take, with hipIpc-mapped regions instead of same-process pointers). SURVEY 8(e): k = 1 must reproduce the single
learner on the concatenated batch -- here the oracle with minibatches of 2 x 128 = 256 rows."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import parity
import replica_group as RG
from parity import L, O, crux

pytestmark = pytest.mark.gpu


def _shard(seed, E=8, T=128):
    extras = ["return", "logprob", "advantage"]
    _, oa = parity.make_pair(parity.ACTOR_DIMS, parity.ACTS, 50, 0, "discrete")
    _, oc = parity.make_pair(parity.CRITIC_DIMS, parity.ACTS, 50, 1)
    ob = O.OBuffer(4, 2, L.ACTION_DISCRETE, E * T, extras)
    O.OEnv("cartpole", E, 60, 0.99, seed).rollout(oa, parity.rollout_cfg(), ob, T)
    O.chk(O.lib().orc_fill_gae(ob.h, oc.h, 0.95, 0.99)); O.chk(O.lib().orc_fill_returns(ob.h, 0.99)); O.chk(O.lib().orc_whiten(ob.h, L.COL["advantage"]))
    return {k: ob[k] for k in ob.keys()}


def _interleave(shards, bs):
    """row (rank r, position j) of the global buffer: minibatch j // bs holds [bs rows of rank 0 | bs rows of rank 1 | ...]."""
    R, N = len(shards), shards[0]["s"].shape[1]
    pos = np.empty((R, N), np.int64)
    for r in range(R):
        j = np.arange(N); pos[r] = (j // bs) * (R * bs) + r * bs + (j % bs)
    out = {}
    for k in shards[0]:
        rows = shards[0][k].shape[0]; a = np.empty((rows, R * N), shards[0][k].dtype, order="F")
        for r in range(R):
            a[:, pos[r]] = shards[r][k]
        out[k] = a
    return out, pos


@pytest.fixture()
def two_contexts(gpu_ctx):
    c1 = crux.Context(0)
    RG.attach_or_skip([gpu_ctx, c1], owned=[c1])
    yield gpu_ctx, c1
    gpu_ctx.peer_detach(); c1.peer_detach(); c1.close()


_bound = RG.bound
_run_threads = RG.run_threads_raise


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_two_replicas_equal_the_single_learner_on_the_concatenated_batch(two_contexts, which):
    ctxs = two_contexts; bs, epochs = 128, 2
    shards = [_shard(200), _shard(201)]
    N = shards[0]["s"].shape[1]; extras = ["return", "logprob", "advantage"]
    dims = parity.ACTOR_DIMS if which == "actor" else parity.CRITIC_DIMS
    loss, head = ("ppo", "categorical") if which == "actor" else ("value_mse", "deterministic")
    rng = np.random.default_rng(5)
    perms = [np.stack([rng.permutation(N) for _ in range(epochs)]) for _ in range(2)]          # every replica shuffles its own shard (0-based)
    nets, bufs = [], []
    for r, ctx in enumerate(ctxs):
        ch = parity.chain(dims, parity.ACTS)
        g = crux.DiscreteNetwork(ch, [1, 2], ctx=ctx, seed=77, stream=3) if which == "actor" else crux.ContinuousNetwork(ch, ctx=ctx, seed=77, stream=3)
        b = crux.ExperienceBuffer(crux.ContinuousSpace(4), crux.DiscreteSpace(2), N, extras, ctx=ctx); b.push_(shards[r])
        nets.append(g); bufs.append(b)
    assert np.array_equal(nets[0].get_params(), nets[1].get_params())
    P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
    infos = [None, None]
    def make(r):
        def f():
            opt = crux.TrainingParams(loss=crux.ppo_loss if which == "actor" else crux.value_mse_loss, batch_size=bs, epochs=epochs, name="n_")
            infos[r] = crux.batch_train_(nets[r], opt, P, bufs[r], perms=perms[r] + 1)
        return f
    _run_threads([make(0), make(1)])
    p0, p1 = nets[0].get_params(), nets[1].get_params()
    assert np.array_equal(p0, p1)                                                    # replicas never diverge: identical sums, identical Adam
    m0, v0, bp0 = nets[0].adam_state(); m1, v1, bp1 = nets[1].adam_state()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(bp0, bp1)
    assert infos[0]["n_batches_trained"] == infos[1]["n_batches_trained"] == epochs * (N // bs)
    assert infos[0]["n_loss"] == infos[1]["n_loss"] and infos[0]["n_grad_norm"] == infos[1]["n_grad_norm"]     # the statistics are global
    # ---- the oracle: ONE learner, minibatches of 256 = [128 rows of replica 0 | 128 rows of replica 1]
    glob, pos = _interleave(shards, bs)
    ob = O.OBuffer(4, 2, L.ACTION_DISCRETE, 2 * N, extras); ob.push(glob)
    o = O.OMlp(dims, parity.ACTS).init_glorot(77, 3).adam_init(float(np.float32(3e-4)))
    assert np.array_equal(o.params, crux.ContinuousNetwork(parity.chain(dims, parity.ACTS), ctx=ctxs[0], seed=77, stream=3).get_params())
    gperm = np.empty((epochs, 2 * N), np.int64)
    for e in range(epochs):
        for r in range(2):
            gperm[e, pos[r]] = pos[r][perms[r][e]]                                    # new[pos(r, j)] = old[pos(r, perm_r[j])]
    cfg = parity.train_cfg(loss, head, 2 * bs, epochs, -1.0, 0)
    oi = np.zeros(L.INFO_N, np.float32)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(gperm), O.vpz(oi), None))
    d = float(np.abs(p0 - o.params).max())
    print(which, "two replicas vs concatenated-batch oracle after %d steps: max |dtheta| = %.3g" % (epochs * (N // bs), d), "loss", infos[0]["n_loss"], float(oi[0]))
    assert d < parity.window_tol(0)
    assert abs(infos[0]["n_loss"] - float(oi[0])) < 2e-5 * max(1.0, abs(float(oi[0])))
    assert abs(infos[0]["n_grad_norm"] - float(oi[1])) < 2e-5 * max(1.0, abs(float(oi[1])))


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_two_replicas_on_identical_shards_reproduce_the_ungrouped_learner(two_contexts, which):
    """N = 2 with the SAME rows and shuffles on both replicas: g + g and the division by two are exact, so the group must leave exactly the parameters an un-grouped learner
    reaches on that shard, bit for bit (bench.py --selftest checks the same across real devices)."""
    ctxs = two_contexts; bs, epochs = 128, 2
    shard = _shard(210); N = shard["s"].shape[1]; extras = ["return", "logprob", "advantage"]
    dims = parity.ACTOR_DIMS if which == "actor" else parity.CRITIC_DIMS
    rng = np.random.default_rng(6); perms = np.stack([rng.permutation(N) for _ in range(epochs)])
    P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
    def mk(ctx):
        ch = parity.chain(dims, parity.ACTS)
        g = crux.DiscreteNetwork(ch, [1, 2], ctx=ctx, seed=79, stream=3) if which == "actor" else crux.ContinuousNetwork(ch, ctx=ctx, seed=79, stream=3)
        b = crux.ExperienceBuffer(crux.ContinuousSpace(4), crux.DiscreteSpace(2), N, extras, ctx=ctx); b.push_(shard)
        return g, b
    pairs = [mk(c) for c in ctxs]
    def make(r):
        def f():
            opt = crux.TrainingParams(loss=crux.ppo_loss if which == "actor" else crux.value_mse_loss, batch_size=bs, epochs=epochs, name="n_")
            crux.batch_train_(pairs[r][0], opt, P, pairs[r][1], perms=perms + 1)
        return f
    _run_threads([make(0), make(1)])
    c3 = crux.Context(0)
    try:
        g, b = mk(c3)
        crux.batch_train_(g, crux.TrainingParams(loss=crux.ppo_loss if which == "actor" else crux.value_mse_loss, batch_size=bs, epochs=epochs, name="n_"), P, b, perms=perms + 1)
        ref = g.get_params(); got = pairs[0][0].get_params()
        print(which, "identical shards, group of two vs un-grouped: max |d| = %.3g" % float(np.abs(ref - got).max()))
        # (g + g and the division by two are exact, and the learner kernels are compiled without FMA contraction -- csrc/Makefile -- so the group's instantiation forms the
        #  same bits as the un-grouped learner's: bit for bit)
        assert np.array_equal(got, pairs[1][0].get_params()) and np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    finally:
        c3.close()


def _one_learner(ctx, seed=210, which="critic"):
    shard = _shard(seed); N = shard["s"].shape[1]; extras = ["return", "logprob", "advantage"]
    dims = parity.ACTOR_DIMS if which == "actor" else parity.CRITIC_DIMS; ch = parity.chain(dims, parity.ACTS)
    g = crux.DiscreteNetwork(ch, [1, 2], ctx=ctx, seed=79, stream=3) if which == "actor" else crux.ContinuousNetwork(ch, ctx=ctx, seed=79, stream=3)
    b = crux.ExperienceBuffer(crux.ContinuousSpace(4), crux.DiscreteSpace(2), N, extras, ctx=ctx); b.push_(shard)
    opt = crux.TrainingParams(loss=crux.ppo_loss if which == "actor" else crux.value_mse_loss, batch_size=128, epochs=2, name="n_")
    return g, b, opt


def test_the_host_calls_a_waiting_launch_off(two_contexts):
    """bound 4 of csrc/peer_wait.h (VERDICT r5 #1c): replica 0 trains, replica 1 never does -- the learner's workgroups wait for a flag that will not come (timeout 30 s, budget
    off). crux_peer_abort from another host thread -- no GPU work, while the training call sits in its stream synchronisation -- ends the launch: CRUX_EHIP within moments, the
    message names the host; the device is usable afterwards."""
    import time
    c0, c1 = two_contexts
    c0.peer_set_timeout_ms(30000); c0.peer_set_budget_ms(0)
    g, b, opt = _one_learner(c0)
    box = {}
    def train():
        t0 = time.time()
        try:
            crux.batch_train_(g, opt, {}, b)
        except crux.CruxError as e:
            box["err"] = e
        box["seconds"] = time.time() - t0
    t = threading.Thread(target=train, daemon=True); t.start()
    time.sleep(0.5); assert t.is_alive(), "the learner did not wait for its peer: %r" % box
    c0.peer_abort(); t.join(10.0)
    assert not t.is_alive(), "the launch did not end after crux_peer_abort"
    print("host abort: the call returned after %.2f s: %s" % (box["seconds"], box.get("err")))
    assert box.get("err") is not None and box["err"].code == L.EHIP and "host called the launch off" in str(box["err"]) and box["seconds"] < 5.0
    assert c0.peer_abort_reason()[0] == 4
    c0.peer_abort_clear()
    p = g.get_params(); assert np.isfinite(p).all()          # nothing was applied, the context answers


def test_the_launch_budget_ends_a_group_whose_peer_is_slow(two_contexts):
    """bound 2: replica 1 starts a second late. The per-exchange timeout (30 s) would sit that out; the launch budget (300 ms for all waits of one launch together) does not:
    replica 0 gives up with CRUX_EHIP naming the budget and tells its peer, which leaves as soon as it starts -- the regime of replicas whose queues are time-sliced, where
    every exchange is answered a scheduling quantum late (profiles/r06_same_device_oversubscription.txt)."""
    import time
    ctxs = two_contexts
    for c in ctxs:
        c.peer_set_timeout_ms(30000); c.peer_set_budget_ms(300)
    L0, L1 = _one_learner(ctxs[0]), _one_learner(ctxs[1])
    secs = [None, None]
    def make(r, delay):
        def f():
            time.sleep(delay); t0 = time.time()
            try:
                crux.batch_train_((L0, L1)[r][0], (L0, L1)[r][2], {}, (L0, L1)[r][1])
            finally:
                secs[r] = time.time() - t0
        return f
    errs = RG.run_threads([make(0, 0.0), make(1, 1.0)], seconds=30.0)
    print("budget: replica 0 after %.2f s: %s | replica 1 after %.2f s: %s" % (secs[0], errs[0], secs[1], errs[1]))
    assert errs[0] is not None and errs[0].code == L.EHIP and "budget" in str(errs[0]) and 0.25 < secs[0] < 2.0      # (300 ms of waiting + the call's own setup; measured 0.30 s)
    assert errs[1] is not None and errs[1].code == L.EHIP and secs[1] < 5.0          # told by replica 0's abort word: it does not wait for its own timeout
    assert ctxs[1].peer_abort_reason()[0] == 2


def test_the_rendezvous_probe(two_contexts):
    """crux_peer_probe (collective; crux_peer_attach_local already ran it once): both replicas' kernels meet in microseconds on every learner stream. A probe only ONE rank
    calls cannot meet anybody: CRUX_EHIP within its bounds, and the group refuses further probes until it is attached again."""
    import time
    ctxs = two_contexts; res = [None, None]
    def make(r):
        def f():
            res[r] = ctxs[r].peer_probe(rounds=256, first_bound_ms=2000, round_bound_ms=20)
        return f
    _run_threads([make(0), make(1)])
    print("rendezvous probe, us [first round, slowest later round] x 2 streams:", res)
    for r in range(2):
        assert max(res[r][1], res[r][3]) < 1000.0, res          # measured 0.8-1.0 us; time-sliced queues answer after 20 000-50 000 us
    t0 = time.time()
    with pytest.raises(crux.CruxError) as e:
        ctxs[0].peer_probe(rounds=16, first_bound_ms=100, round_bound_ms=20)
    assert e.value.code == L.EHIP and "did not meet" in str(e.value) and time.time() - t0 < 3.0
    with pytest.raises(crux.CruxError) as e2:
        ctxs[0].peer_probe(rounds=16, first_bound_ms=100, round_bound_ms=20)
    assert e2.value.code == L.EINVAL


def _group(gpu_ctx, R, attempts=5):
    """R contexts on device 0 wired into a replica group. Four replicas need all eight hardware queues (a learner and an auxiliary stream each): crux_peer_attach_local sometimes
    cannot place them and says so -- fresh contexts get fresh streams, so the attach is retried; if the placement never works the test is skipped with the library's message."""
    last = None
    for _ in range(attempts):
        extra = [crux.Context(0) for _ in range(R - 1)]; ctxs = [gpu_ctx] + extra
        try:
            crux.peer_attach_local(ctxs)
            _bound(ctxs)
            return ctxs, extra
        except crux.CruxError as e:
            last = e
            for c in ctxs:
                try:
                    c.peer_detach()
                except Exception:       # noqa: BLE001
                    pass
            for c in extra:
                c.close()
            if "hardware queue" not in str(e):
                raise
    pytest.skip("no placement of %d replicas on the device's hardware queues after %d attempts: %s" % (R, attempts, last))


def _local_sgd_twin(R, shards, perms, dims, loss, head, bs, epochs, k, seed, stream):
    """the oracle twin of the in-kernel periodic form: R oracle learners, each on its own shard and shuffle, take k local minibatch steps (training.jl:40-43 on the composed shuffle order), then theta, m and v are replaced by the mean over the replicas -- float32 sum in rank order times float32(1 / R), the kernel's arithmetic."""
    N = shards[0]["s"].shape[1]; extras = ["return", "logprob", "advantage"]; nmb = N // bs
    os_, obs = [], []
    for r in range(R):
        ob = O.OBuffer(4, 2, L.ACTION_DISCRETE, N, extras); ob.push(shards[r]); obs.append(ob)
        os_.append(O.OMlp(dims, parity.ACTS).init_glorot(seed, stream).adam_init(float(np.float32(3e-4))))
    inv = np.float32(1.0) / np.float32(R)
    def mean(xs):
        acc = xs[0].astype(np.float32).copy()
        for x in xs[1:]:
            acc = acc + x
        return acc * inv
    oi = np.zeros(L.INFO_N, np.float32)
    cfg = parity.train_cfg(loss, head, bs, 1, -1.0, 0)
    order = [np.arange(N, dtype=np.int64) for _ in range(R)]
    for e in range(epochs):
        for r in range(R):
            order[r] = order[r][perms[r][e]]                       # shuffle!(D) composes (experience_buffer.jl:118-124): the rows of epoch e in buffer coordinates
        for c0 in range(0, nmb, k):
            for r in range(R):
                for j in range(c0, c0 + k):
                    ids = np.ascontiguousarray(order[r][j * bs:(j + 1) * bs])
                    O.chk(O.lib().orc_train_step(os_[r].h, obs[r].h, C.byref(cfg), O.vpz(ids), bs, O.vpz(oi)))
            th = mean([o.params for o in os_]); st = [o.adam_state() for o in os_]
            m = mean([x[0] for x in st]); v = mean([x[1] for x in st])
            for o in os_:
                o.params[:] = th; o.set_adam_state(m, v)
    return os_[0]


_PERIODIC = [(2, 8, "actor"), (2, 8, "critic"), (2, 4, "actor"), (3, 4, "critic"), (4, 4, "critic")] + ([(2, 2, "actor"), (2, 4, "critic"), (2, 2, "critic"), (3, 4, "actor"), (3, 8, "actor")] if os.environ.get("CRUX_TEST_PERIODIC_ALL") else []) + ([(4, 4, "critic"), (4, 8, "actor")] if os.environ.get("CRUX_TEST_FOUR_REPLICAS") else [])


@pytest.mark.parametrize("R,k,which", _PERIODIC)
def test_periodic_form_equals_the_local_sgd_twin(gpu_ctx, R, k, which):
    """crux_peer_set_sync_every(k > 1): R persistent learners take LOCAL Adam steps on their shards and average theta, m, v through the peer slots after every k-th step inside
    the kernel (train_fs_kernel.h). Replicas must leave every call bit-identical; the oracle's local-SGD twin bounds the values (within 1e-6)."""
    ctxs, extra = _group(gpu_ctx, R)
    try:
        for c in ctxs:
            c.peer_set_sync_every(k)
        bs, epochs = 128, 2
        shards = [_shard(700 + r, E=8, T=128) for r in range(R)]
        N = shards[0]["s"].shape[1]; extras = ["return", "logprob", "advantage"]
        assert (N // bs) % k == 0
        dims = parity.ACTOR_DIMS if which == "actor" else parity.CRITIC_DIMS
        loss, head = ("ppo", "categorical") if which == "actor" else ("value_mse", "deterministic")
        rng = np.random.default_rng(9)
        perms = [np.stack([rng.permutation(N) for _ in range(epochs)]) for _ in range(R)]
        nets, bufs = [], []
        for r, ctx in enumerate(ctxs):
            ch = parity.chain(dims, parity.ACTS)
            g = crux.DiscreteNetwork(ch, [1, 2], ctx=ctx, seed=81, stream=3) if which == "actor" else crux.ContinuousNetwork(ch, ctx=ctx, seed=81, stream=3)
            b = crux.ExperienceBuffer(crux.ContinuousSpace(4), crux.DiscreteSpace(2), N, extras, ctx=ctx); b.push_(shards[r])
            nets.append(g); bufs.append(b)
        P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
        infos = [None] * R
        def make(r):
            def f():
                opt = crux.TrainingParams(loss=crux.ppo_loss if which == "actor" else crux.value_mse_loss, batch_size=bs, epochs=epochs, name="n_")
                infos[r] = crux.batch_train_(nets[r], opt, P, bufs[r], perms=perms[r] + 1)
            return f
        _run_threads([make(r) for r in range(R)])
        ps = [n.get_params() for n in nets]; ad = [n.adam_state() for n in nets]
        for r in range(1, R):
            assert np.array_equal(ps[0], ps[r]) and np.array_equal(ad[0][0], ad[r][0]) and np.array_equal(ad[0][1], ad[r][1]) and np.array_equal(ad[0][2], ad[r][2])
        assert all(i["n_batches_trained"] == epochs * (N // bs) for i in infos)
        o = _local_sgd_twin(R, shards, perms, dims, loss, head, bs, epochs, k, 81, 3)
        d = float(np.abs(ps[0] - o.params).max()); om, ov, _ = o.adam_state()
        dm, dv = float(np.abs(ad[0][0] - om).max()), float(np.abs(ad[0][1] - ov).max())
        print("periodic form R=%d k=%d %s after %d steps: max |dtheta| = %.3g  |dm| = %.3g  |dv| = %.3g vs the local-SGD oracle twin" % (R, k, which, epochs * (N // bs), d, dm, dv))
        assert d < 1e-6 and dm < 1e-6 * max(1.0, float(np.abs(om).max())) and dv < 1e-6 * max(1.0, float(np.abs(ov).max()))      # (the critic's moments are O(10): relative there)
        # a call the periodic form cannot keep in lock step is refused
        with pytest.raises(crux.CruxError) as e:
            crux.batch_train_(nets[0], crux.TrainingParams(loss=crux.ppo_loss if which == "actor" else crux.value_mse_loss, batch_size=bs, epochs=1, max_batches=3, name="n_"), P, bufs[0])
        assert e.value.code == L.EINVAL
    finally:
        for c in ctxs:
            try:
                c.peer_set_sync_every(1); c.peer_detach()
            except Exception:       # noqa: BLE001
                pass
        for c in extra:
            c.close()


def test_policy_gradient_training_of_two_replicas_with_kl_early_stopping(two_contexts):
    """actor and critic of both replicas (four persistent kernels, two exchange streams per replica) through crux_policy_gradient_training; the KL
    statistic is all-reduced with the gradient, so both replicas stop at the same minibatch and stay bit-identical."""
    ctxs = two_contexts; bs = 128
    shards = [_shard(300), _shard(301)]
    N = shards[0]["s"].shape[1]; extras = ["return", "logprob", "advantage"]
    sv, bufs = [], []
    for r, ctx in enumerate(ctxs):
        a = crux.DiscreteNetwork(parity.chain(parity.ACTOR_DIMS, parity.ACTS), [1, 2], ctx=ctx, seed=9, stream=0)
        c = crux.ContinuousNetwork(parity.chain(parity.CRITIC_DIMS, parity.ACTS), ctx=ctx, seed=9, stream=1)
        b = crux.ExperienceBuffer(crux.ContinuousSpace(4), crux.DiscreteSpace(2), N, extras, ctx=ctx); b.push_(shards[r])
        class _S:
            pass
        s = _S(); s.agent = crux.PolicyParams(crux.ActorCritic(a, c)); s.P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
        s.a_opt = crux.TrainingParams(loss=crux.ppo_loss, batch_size=bs, epochs=6, target_kl=0.004, name="actor_", shuffle_seed=40 + r)
        s.c_opt = crux.TrainingParams(loss=crux.value_mse_loss, batch_size=bs, epochs=3, name="critic_", shuffle_seed=60 + r)
        sv.append(s); bufs.append(b)
    for tk in (0.004, None):           # sequential path with early stopping, then the concurrent actor || critic path
        infos = [None, None]
        for s in sv:
            s.a_opt.target_kl = tk
        def make(r):
            def f():
                infos[r] = crux.policy_gradient_training(sv[r], bufs[r])
            return f
        _run_threads([make(0), make(1)])
        A0, A1 = sv[0].agent.pi.A, sv[1].agent.pi.A; C0, C1 = sv[0].agent.pi.C, sv[1].agent.pi.C
        assert np.array_equal(A0.get_params(), A1.get_params()) and np.array_equal(C0.get_params(), C1.get_params())
        assert infos[0]["actor_batches_trained"] == infos[1]["actor_batches_trained"] and infos[0]["kl"] == infos[1]["kl"]
        if tk is not None:
            assert infos[0]["actor_batches_trained"] < 6 * (N // bs)              # the KL stop fired (on the same minibatch in both replicas)
        else:
            assert infos[0]["actor_batches_trained"] == 6 * (N // bs) and infos[0]["critic_batches_trained"] == 3 * (N // bs)


def test_policy_gradient_training_of_two_replicas_in_the_periodic_form(two_contexts):
    """crux_policy_gradient_training under crux_peer_set_sync_every(8): actor and critic of both replicas train concurrently (four persistent kernels, periodic exchanges on both
    learner streams) and leave the call bit-identical across the replicas; KL early stopping is refused in this form (the statistics are local between exchanges)."""
    ctxs = two_contexts; bs = 128
    shards = [_shard(310), _shard(311)]
    N = shards[0]["s"].shape[1]; extras = ["return", "logprob", "advantage"]
    sv, bufs = [], []
    for r, ctx in enumerate(ctxs):
        ctx.peer_set_sync_every(8)
        a = crux.DiscreteNetwork(parity.chain(parity.ACTOR_DIMS, parity.ACTS), [1, 2], ctx=ctx, seed=9, stream=0)
        c = crux.ContinuousNetwork(parity.chain(parity.CRITIC_DIMS, parity.ACTS), ctx=ctx, seed=9, stream=1)
        b = crux.ExperienceBuffer(crux.ContinuousSpace(4), crux.DiscreteSpace(2), N, extras, ctx=ctx); b.push_(shards[r])
        class _S:
            pass
        s = _S(); s.agent = crux.PolicyParams(crux.ActorCritic(a, c)); s.P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
        s.a_opt = crux.TrainingParams(loss=crux.ppo_loss, batch_size=bs, epochs=4, target_kl=None, name="actor_", shuffle_seed=40 + r)
        s.c_opt = crux.TrainingParams(loss=crux.value_mse_loss, batch_size=bs, epochs=4, name="critic_", shuffle_seed=60 + r)
        sv.append(s); bufs.append(b)
    try:
        infos = [None, None]
        def make(r):
            def f():
                infos[r] = crux.policy_gradient_training(sv[r], bufs[r])
            return f
        _run_threads([make(0), make(1)])
        A0, A1 = sv[0].agent.pi.A, sv[1].agent.pi.A; C0, C1 = sv[0].agent.pi.C, sv[1].agent.pi.C
        assert np.array_equal(A0.get_params(), A1.get_params()) and np.array_equal(C0.get_params(), C1.get_params())
        assert all(np.array_equal(x, y) for x, y in zip(A0.adam_state(), A1.adam_state()))
        assert infos[0]["actor_batches_trained"] == infos[1]["actor_batches_trained"] == 4 * (N // bs)
        sv[0].a_opt.target_kl = 0.004
        with pytest.raises(crux.CruxError) as e:
            crux.policy_gradient_training(sv[0], bufs[0])
        assert e.value.code == L.EINVAL
    finally:
        for ctx in ctxs:
            ctx.peer_set_sync_every(1)


def test_unsupported_shape_with_a_group_attached_is_refused(two_contexts):
    """the exchange lives in k_train_fs2's replica-group forms and the dense-engine learner: a learner neither covers must fail loudly instead of training un-synchronised."""
    ctx = two_contexts[0]
    g = crux.ContinuousNetwork(parity.chain([4, 32, 1], ["relu", "identity"]), ctx=ctx)
    d = _shard(400, E=2, T=64)
    b = crux.ExperienceBuffer(crux.ContinuousSpace(4), crux.DiscreteSpace(2), 128, ["return", "logprob", "advantage"], ctx=ctx); b.push_(d)
    with pytest.raises(crux.CruxError) as e:
        crux.batch_train_(g, crux.TrainingParams(loss=crux.value_mse_loss, batch_size=32, epochs=1), {}, b)
    assert e.value.code == L.EUNSUP


# Four replicas on ONE device need a learner and an auxiliary stream per context = all eight hardware queues (GPU_MAX_HW_QUEUES = 8; larger values do not help): now and
# then crux_peer_attach_local cannot find such a placement in its eight attempts and reports it: _group retries with fresh contexts (round 4: N = 4 runs by default, the
# exchange is also covered at N = 4 by tests/peer_stress.py); N = 3 covers the unpaired last rank and the split of the peers between a learner's two workgroups.
_RS = [(3, "actor"), (3, "critic"), (4, "critic")] + ([(4, "actor")] if os.environ.get("CRUX_TEST_FOUR_REPLICAS") else [])


@pytest.mark.parametrize("R,which", _RS)
def test_more_than_two_replicas_sum_in_rank_order(gpu_ctx, R, which):
    """N = 3 (an unpaired last rank in the slot loop) and N = 4 (peers shared between the two workgroups of a learner) on one GPU: R persistent learners spin
    concurrently, every step adds R contributions in rank order; all replicas stay bit-identical and equal the oracle's single learner on R x 128 rows."""
    ctxs, extra = _group(gpu_ctx, R)
    try:
        bs, epochs = 128, 1
        shards = [_shard(500 + r, E=4, T=128) for r in range(R)]
        N = shards[0]["s"].shape[1]; extras = ["return", "logprob", "advantage"]
        dims = parity.ACTOR_DIMS if which == "actor" else parity.CRITIC_DIMS
        loss, head = ("ppo", "categorical") if which == "actor" else ("value_mse", "deterministic")
        rng = np.random.default_rng(7)
        perms = [np.stack([rng.permutation(N) for _ in range(epochs)]) for _ in range(R)]
        nets, bufs = [], []
        for r, ctx in enumerate(ctxs):
            ch = parity.chain(dims, parity.ACTS)
            g = crux.DiscreteNetwork(ch, [1, 2], ctx=ctx, seed=78, stream=3) if which == "actor" else crux.ContinuousNetwork(ch, ctx=ctx, seed=78, stream=3)
            b = crux.ExperienceBuffer(crux.ContinuousSpace(4), crux.DiscreteSpace(2), N, extras, ctx=ctx); b.push_(shards[r])
            nets.append(g); bufs.append(b)
        P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
        def make(r):
            def f():
                opt = crux.TrainingParams(loss=crux.ppo_loss if which == "actor" else crux.value_mse_loss, batch_size=bs, epochs=epochs, name="n_")
                crux.batch_train_(nets[r], opt, P, bufs[r], perms=perms[r] + 1)
            return f
        _run_threads([make(r) for r in range(R)])
        ps = [n.get_params() for n in nets]
        for r in range(1, R):
            assert np.array_equal(ps[0], ps[r]), "replica %d diverged" % r
        glob, pos = _interleave(shards, bs)
        ob = O.OBuffer(4, 2, L.ACTION_DISCRETE, R * N, extras); ob.push(glob)
        o = O.OMlp(dims, parity.ACTS).init_glorot(78, 3).adam_init(float(np.float32(3e-4)))
        gperm = np.empty((epochs, R * N), np.int64)
        for e in range(epochs):
            for r in range(R):
                gperm[e, pos[r]] = pos[r][perms[r][e]]
        cfg = parity.train_cfg(loss, head, R * bs, epochs, -1.0, 0); oi = np.zeros(L.INFO_N, np.float32)
        O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(gperm), O.vpz(oi), None))
        d = float(np.abs(ps[0] - o.params).max())
        print(which, "%d replicas vs the concatenated-batch oracle after %d steps: max |dtheta| = %.3g" % (R, epochs * (N // bs), d))
        assert d < parity.window_tol(0)
    finally:
        for c in ctxs:
            try:
                c.peer_detach()
            except Exception:       # noqa: BLE001
                pass
        for c in extra:
            c.close()


def test_three_replicas_of_the_c5_actor(gpu_ctx):
    """the wide-head (17 -> 64 -> 64 -> 6, tanh, Gaussian) form of the exchange, which takes the peer slots one rank at a time: 3 replicas == the oracle on 3 x 128 rows"""
    R, bs, E, T = 3, 128, 4, 128
    od, ad, disc, adims, cdims, acts, kind, head, okind = parity.FAMILIES["synth_c5"]
    extras = ["return", "logprob", "advantage"]
    def shard(seed):
        _, oa = parity.make_pair(adims, acts, 50, 0, kind, n_extra=ad, extra_init=-0.5); _, oc = parity.make_pair(cdims, acts, 50, 1)
        ob = O.OBuffer(od, ad, L.ACTION_CONTINUOUS, E * T, extras)
        O.OEnv(okind, E, 60, 0.99, seed, so=od, sa=ad).rollout(oa, parity.rollout_cfg(head=head), ob, T)
        O.chk(O.lib().orc_fill_gae(ob.h, oc.h, 0.95, 0.99)); O.chk(O.lib().orc_fill_returns(ob.h, 0.99)); O.chk(O.lib().orc_whiten(ob.h, L.COL["advantage"]))
        return {k: ob[k] for k in ob.keys()}
    ctxs, extra = _group(gpu_ctx, R)
    try:
        shards = [shard(600 + r) for r in range(R)]; N = E * T
        rng = np.random.default_rng(9); perms = [rng.permutation(N)[None, :] for _ in range(R)]
        nets, bufs = [], []
        for r, ctx in enumerate(ctxs):
            g = crux.GaussianPolicy(parity.chain(adims, acts), np.full(ad, -0.5, np.float32), ctx=ctx, seed=79, stream=3)
            b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), N, extras, ctx=ctx); b.push_(shards[r])
            nets.append(g); bufs.append(b)
        P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.0}
        def make(r):
            def f():
                crux.batch_train_(nets[r], crux.TrainingParams(loss=crux.ppo_loss, batch_size=bs, epochs=1, name="n_"), P, bufs[r], perms=perms[r] + 1)
            return f
        _run_threads([make(r) for r in range(R)])
        ps = [n.get_params() for n in nets]
        assert np.array_equal(ps[0], ps[1]) and np.array_equal(ps[0], ps[2])
        glob, pos = _interleave(shards, bs)
        ob = O.OBuffer(od, ad, L.ACTION_CONTINUOUS, R * N, extras); ob.push(glob)
        o = O.OMlp(adims, acts, ad).init_glorot(79, 3, -0.5).adam_init(float(np.float32(3e-4)))
        gperm = np.empty((1, R * N), np.int64)
        for r in range(R):
            gperm[0, pos[r]] = pos[r][perms[r][0]]
        cfg = parity.train_cfg("ppo", "gaussian", R * bs, 1, -1.0, 0, le=0.0); oi = np.zeros(L.INFO_N, np.float32)
        O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(gperm), O.vpz(oi), None))
        d = float(np.abs(ps[0] - o.params).max())
        print("c5 actor, 3 replicas vs the concatenated-batch oracle after %d steps: max |dtheta| = %.3g" % (N // bs, d))
        assert d < parity.window_tol(0)
    finally:
        for c in ctxs:
            try:
                c.peer_detach()
            except Exception:       # noqa: BLE001
                pass
        for c in extra:
            c.close()


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_dense_engine_learner_under_a_replica_group_equals_the_concatenated_batch_oracle(two_contexts, which):
    """replica groups for the shapes the dense engine serves. 8->128->128->4 PPO actor / 8->128->128->1 critic (outside the register-resident family: ~13
    launches per minibatch, train_dense.hip) under a group of two: the flat gradient (18 180 floats = three slot-sized chunks) and the head's statistics are SUM-all-reduced
    by k_px_allreduce_flat between the pullback and the gated Adam. Two replicas with minibatches of 128 must take the steps of ONE oracle learner on minibatches of 256 and
    stay bit-identical to each other."""
    _group_vs_concatenated_oracle(two_contexts, which, 8, 128, 4, 31, "dense-engine learner")


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_c2_learner_under_a_replica_group_without_the_feature_split_kernel_takes_the_dense_engine(two_contexts, monkeypatch, which):
    """CRUX_FS=0 switches k_train_fs2 off; the one- and two-CU kernels have no replica-group exchange, so a grouped 4->64->64->2 PPO actor / 4->64->64->1 critic with minibatches
    of 128 is the dense-engine learner's (train_dense.hip, k_px_allreduce_flat). Same checks as above: bit-identical replicas, the concatenated-batch oracle within the same bounds.
    (The monkeypatch fixture re-reads the process-wide switches after the setenv and again after the test.)"""
    monkeypatch.setenv("CRUX_FS", "0")
    _group_vs_concatenated_oracle(two_contexts, which, 4, 64, 2, 37, "C2 learner under CRUX_FS=0")


def _group_vs_concatenated_oracle(ctxs, which, od, width, na, seed, what):
    bs, epochs, N = 128, 2, 512
    rng = np.random.default_rng(seed); extras = ["return", "logprob", "advantage"]
    def shard():
        ai = rng.integers(0, na, N)
        return {"s": rng.normal(0, 1, (od, N)).astype(np.float32), "a": np.eye(na, dtype=bool)[:, ai], "sp": rng.normal(0, 1, (od, N)).astype(np.float32), "r": np.ones((1, N), np.float32),
                "done": np.zeros((1, N), bool), "episode_end": np.zeros((1, N), bool), "return": rng.normal(0, 1, (1, N)).astype(np.float32),
                "logprob": rng.normal(-1.4, 0.05, (1, N)).astype(np.float32), "advantage": rng.normal(0, 1, (1, N)).astype(np.float32)}
    shards = [shard(), shard()]
    dims = [od, width, width, na] if which == "actor" else [od, width, width, 1]
    loss, head = ("ppo", "categorical") if which == "actor" else ("value_mse", "deterministic")
    perms = [np.stack([rng.permutation(N) for _ in range(epochs)]) for _ in range(2)]
    nets, bufs = [], []
    for r, ctx in enumerate(ctxs):
        ch = parity.chain(dims, parity.ACTS)
        g = crux.DiscreteNetwork(ch, list(range(1, na + 1)), ctx=ctx, seed=78, stream=3) if which == "actor" else crux.ContinuousNetwork(ch, ctx=ctx, seed=78, stream=3)
        b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(na), N, extras, ctx=ctx); b.push_(shards[r])
        nets.append(g); bufs.append(b)
    P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
    infos = [None, None]
    def make(r):
        def f():
            opt = crux.TrainingParams(loss=crux.ppo_loss if which == "actor" else crux.value_mse_loss, batch_size=bs, epochs=epochs, name="n_")
            infos[r] = crux.batch_train_(nets[r], opt, P, bufs[r], perms=perms[r] + 1)
        return f
    _run_threads([make(0), make(1)])
    p0, p1 = nets[0].get_params(), nets[1].get_params()
    assert np.array_equal(p0, p1)
    m0, v0, bp0 = nets[0].adam_state(); m1, v1, bp1 = nets[1].adam_state()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(bp0, bp1)
    assert infos[0]["n_loss"] == infos[1]["n_loss"] and infos[0]["n_grad_norm"] == infos[1]["n_grad_norm"]
    glob, pos = _interleave(shards, bs)
    ob = O.OBuffer(od, na, L.ACTION_DISCRETE, 2 * N, extras); ob.push(glob)
    o = O.OMlp(dims, parity.ACTS).init_glorot(78, 3).adam_init(float(np.float32(3e-4)))
    gperm = np.empty((epochs, 2 * N), np.int64)
    for e in range(epochs):
        for r in range(2):
            gperm[e, pos[r]] = pos[r][perms[r][e]]
    cfg = parity.train_cfg(loss, head, 2 * bs, epochs, -1.0, 0)
    oi = np.zeros(L.INFO_N, np.float32)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(gperm), O.vpz(oi), None))
    d = float(np.abs(p0 - o.params).max())
    print(which, what + ", two replicas vs concatenated-batch oracle after %d steps: max |dtheta| = %.3g" % (epochs * (N // bs), d), "loss", infos[0]["n_loss"], float(oi[0]))
    assert d < 2e-6            # measured 4.5e-8 (actor) / 1.5e-8 (critic) after 8 steps on the 128-wide shapes
    assert abs(infos[0]["n_loss"] - float(oi[0])) < 2e-5 * max(1.0, abs(float(oi[0])))


@pytest.mark.parametrize("dims", [[8, 128, 128, 4], [4, 64, 64, 2]], ids=["128wide", "cartpole64"])
def test_lagrange_ppo_under_a_replica_group_equals_the_concatenated_batch_oracle(two_contexts, dims):
    """LagrangePPO with a group attached (refused until round 3). lagrange_ppo_loss runs its PID penalty controller on the minibatch's average episode cost EVERY time it is
    evaluated (ppo.jl:80-116); under a group the minibatch is the global one, so the two Float64 sums (cost, episode ends) of every rank are exchanged bit for bit through the
    peer slots before the controller step (train_dense.hip: k_lagrange_pid), then the gradient and the statistics as for ppo_loss. Two replicas with minibatches of 128 must take
    the steps of ONE oracle learner on minibatches of 256 -- parameters, controller state, infos -- and stay bit-identical to each other. The 64-wide actor, which runs on the
    register-resident lagrange kernels without a group, takes the dense-engine learner with one."""
    import test_gpu_lagrange as TL
    ctxs = two_contexts; bs, epochs, N = 128, 2, 512; od, na = dims[0], dims[-1]
    rng = np.random.default_rng(41); extras = ["return", "logprob", "advantage", "cost", "cost_advantage", "cost_return"]
    def shard():
        ai = rng.integers(0, na, N)
        return {"s": rng.normal(0, 1, (od, N)).astype(np.float32), "a": np.eye(na, dtype=bool)[:, ai], "sp": rng.normal(0, 1, (od, N)).astype(np.float32), "r": np.ones((1, N), np.float32),
                "done": np.zeros((1, N), bool), "episode_end": rng.random((1, N)) < 0.1, "return": rng.normal(0, 1, (1, N)).astype(np.float32),
                "logprob": rng.normal(-np.log(na), 0.05, (1, N)).astype(np.float32), "advantage": rng.normal(0, 1, (1, N)).astype(np.float32),
                "cost": (rng.random((1, N)) < 0.3).astype(np.float32), "cost_advantage": rng.normal(0, 1, (1, N)).astype(np.float32), "cost_return": rng.normal(1, 0.3, (1, N)).astype(np.float32)}
    shards = [shard(), shard()]
    perms = [np.stack([rng.permutation(N) for _ in range(epochs)]) for _ in range(2)]
    nets, bufs, lags, infos = [], [], [], [None, None]
    for r, ctx in enumerate(ctxs):
        g = crux.DiscreteNetwork(parity.chain(dims, parity.ACTS), list(range(1, na + 1)), ctx=ctx, seed=79, stream=3)
        b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(na), N, extras, ctx=ctx); b.push_(shards[r])
        nets.append(g); bufs.append(b); lags.append(TL._lag())
    def make(r):
        def f():
            P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1, "lagrange": lags[r]}
            infos[r] = crux.batch_train_(nets[r], crux.TrainingParams(loss=crux.lagrange_ppo_loss, batch_size=bs, epochs=epochs, name="actor_"), P, bufs[r], perms=perms[r] + 1)
        return f
    olag = TL._copy_lag(lags[0])
    _run_threads([make(0), make(1)])
    p0, p1 = nets[0].get_params(), nets[1].get_params()
    assert np.array_equal(p0, p1)
    for f in ("I", "Jc_prev", "smooth_delta", "smooth_Jc", "penalty", "cur_cost", "deriv_term"):
        assert getattr(lags[0], f) == getattr(lags[1], f), f
    glob, pos = _interleave(shards, bs)
    ob = O.OBuffer(od, na, L.ACTION_DISCRETE, 2 * N, extras); ob.push(glob)
    o = O.OMlp(dims, parity.ACTS).init_glorot(79, 3).adam_init(float(np.float32(3e-4)))
    gperm = np.empty((epochs, 2 * N), np.int64)
    for e in range(epochs):
        for r in range(2):
            gperm[e, pos[r]] = pos[r][perms[r][e]]
    cfg = parity.train_cfg("lagrange_ppo", "categorical", 2 * bs, epochs, -1.0, 0)
    oi = np.zeros(L.INFO_N, np.float32); oe_ = np.zeros((epochs, L.INFO_N), np.float32)
    O.chk(O.lib().orc_batch_train_lagrange(o.h, ob.h, C.byref(cfg), C.byref(olag), O.vpz(gperm), O.vpz(oi), O.vpz(oe_)))
    d = float(np.abs(p0 - o.params).max())
    print(dims, "lagrange_ppo_loss, two replicas vs concatenated-batch oracle after %d steps: max |dtheta| = %.3g; penalty %.6g / %.6g" % (epochs * (N // bs), d, lags[0].penalty, olag.penalty))
    assert d < 2e-6
    for f in ("I", "Jc_prev", "smooth_delta", "smooth_Jc", "penalty", "cur_cost", "deriv_term"):
        a, b = getattr(lags[0], f), getattr(olag, f)
        assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), (f, a, b)
    assert lags[0].penalty > 0.0
    for k in ("loss", "penalty", "cur_cost", "cost_loss", "p_loss"):
        a, b = float(infos[0][k if k in infos[0] else "actor_" + k]), float(oi[L.INFO[k]])
        assert abs(a - b) < 2e-5 * max(1.0, abs(b)), (k, a, b)
