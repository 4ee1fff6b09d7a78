"""GPU: gradient_penalty and the OnlineIQLearn critic step (crux_gradient_penalty, crux_iq_step, csrc/iq.hip) against the float64 restatement of
tests/iq_reference.py; value_training(OnlineIQLearn) against the manual composition of the entry points; SQIL's demo plumbing with SoftQ and SAC; and a learning
check of OnlineIQLearn on CartPole from the committed demonstrations.

Reference: src/model_free/il/iqlearn.jl, il/sqil.jl, src/extras/gradient_penalty.jl. Tolerances are those of tests/test_gpu_cql.py: 1e-4 relative on losses and
norms, 2e-5 absolute on parameters after one Adam step (entries whose float64 gradient is within 1e-3 of the gradient scale of zero are not compared).
"""
import ctypes as C
import os

import numpy as np
import pytest

import iq_reference as R
import parity
from parity import crux, L

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LR = 1e-3


def _close(a, b, tol=1e-4):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def _qnet(dims, act, seed=5):
    acts = [act] * (len(dims) - 2) + ["identity"]
    return crux.DiscreteNetwork(parity.chain(dims, acts), list(range(1, dims[-1] + 1)), seed=seed, stream=0), acts


def _data(od, A, B, seed=3):
    rng = np.random.default_rng(seed)
    return {"s": rng.normal(0, 1, (od, B)).astype(np.float32), "a": np.eye(A, dtype=bool)[rng.integers(0, A, B)].T.copy(),
            "sp": rng.normal(0, 1, (od, B)).astype(np.float32), "r": rng.normal(0, 1, (1, B)).astype(np.float32), "done": rng.random((1, B)) < 0.2}


def _buffer(ctx, data):
    od, A, B = data["s"].shape[0], data["a"].shape[0], data["s"].shape[1]
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(A), B, ctx=ctx)
    b.push_(data); return b


def _grads(net):
    g = np.empty(net.n_params, np.float32); net.ctx.d2h(net.ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


def _set_grads(net, g):
    net.ctx.h2d(net.ctx.lib.crux_mlp_grads_ptr(net.h), np.ascontiguousarray(g, np.float32))


def _iq_step(net, b, n_policy, gp, reg, seed=11, ctr=7, gamma=0.9, alpha_reg=0.5, lambda_gp=10.0):
    info, iq = np.zeros(L.INFO_N, np.float32), np.zeros(6, np.float32)
    net.ctx.check(net.ctx.lib.crux_iq_step(net.h, b.h, n_policy, gamma, int(reg), alpha_reg, int(gp), lambda_gp, seed, ctr,
                                           info.ctypes.data_as(C.c_void_p), iq.ctypes.data_as(C.c_void_p)))
    return info, iq


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("interp", [False, True])
def test_gradient_penalty_value_and_gradient(gpu_ctx, act, interp):
    ctx, od, B, seed, ctr, lam = gpu_ctx, 6, 50, 21, 4, 3.0
    dims = [od, 48, 40, 3]
    net, acts = _qnet(dims, act)
    rng = np.random.default_rng(1)
    x, xt = rng.normal(0, 1, (od, B)).astype(np.float32), rng.normal(0, 1, (od, B)).astype(np.float32)
    xh = R.xhat(x, xt, R.eps(seed, ctr, B)) if interp else x
    layers = R.mlp_params(net.get_params(), dims)
    P = R.gradient_penalty(layers, acts, xh)
    (lam * P).backward(); g_ref = R.flat_grad(layers)
    v = crux.gradient_penalty(net, x, xt if interp else None, seed=seed, counter=ctr)
    assert _close(v, P.item()), (v, P.item())
    # accumulate: lambda dP/dtheta is ADDED to what the gradient buffer holds
    g0 = rng.normal(0, 1, net.n_params).astype(np.float32); _set_grads(net, g0)
    dx, dxt = ctx.alloc(4 * x.size), ctx.alloc(4 * x.size); ctx.h2d(dx, np.asfortranarray(x)); ctx.h2d(dxt, np.asfortranarray(xt))
    out = np.zeros(1, np.float32)
    ctx.check(ctx.lib.crux_gradient_penalty(net.h, dx, dxt if interp else None, B, 1.0, lam, 1, seed, ctr, out.ctypes.data_as(C.c_void_p)))
    ctx.free(dx); ctx.free(dxt)
    assert _close(out[0], float(P))
    g = _grads(net).astype(np.float64) - g0
    scale = max(1.0, np.abs(g_ref).max())
    assert np.abs(g - g_ref).max() <= 1e-4 * scale, np.abs(g - g_ref).max()


CASES = [(gp, reg, act) for gp in (False, True) for reg in (False, True) for act in ("relu", "tanh")]


@pytest.mark.parametrize("gp,reg,act", CASES, ids=["gp%d-reg%d-%s" % c for c in CASES])
def test_iq_step_matches_reference(gpu_ctx, gp, reg, act):
    ctx, od, A, B, Bp, seed, ctr = gpu_ctx, 5, 3, 64, 32, 11, 7
    dims = [od, 32, 32, A]
    net, acts = _qnet(dims, act)
    net.attach_optimizer(crux.Adam(np.float32(LR)))
    data = _data(od, A, B); b = _buffer(ctx, data)
    p0 = net.get_params()
    layers = R.mlp_params(p0, dims)
    xh = R.xhat(data["s"][:, Bp:], data["s"][:, :Bp], R.eps(seed, ctr, B - Bp))
    loss, ref = R.iq_loss(layers, acts, data["s"], data["a"], data["sp"], data["done"], Bp, gp=gp, reg=reg, xh=xh)
    loss.backward(); g_ref = R.flat_grad(layers)
    info, iq = _iq_step(net, b, Bp, gp, reg, seed, ctr)
    assert _close(info[L.INFO["loss"]], float(loss)), (info[0], float(loss))
    assert _close(info[L.INFO["grad_norm"]], np.linalg.norm(g_ref)), (info[1], np.linalg.norm(g_ref))
    for k, key in enumerate(("softQloss", "valueloss", "avg_R_expert_IQ", "avg_R_demo_IQ", "grad_pen", "reg_loss")):
        assert _close(iq[k], ref[key]), (key, iq[k], ref[key])
    want = R.adam_first_step(p0.astype(np.float64), g_ref, lr=LR)
    ok = np.abs(g_ref) > 1e-3 * np.abs(g_ref).max()
    assert np.abs(net.get_params()[ok] - want[ok]).max() < 2e-5


def test_iq_step_is_deterministic(gpu_ctx):
    ctx, od, A, B = gpu_ctx, 8, 4, 256
    outs = []
    for _ in range(2):
        net, _acts = _qnet([od, 256, 256, A], "tanh", seed=9)
        net.attach_optimizer(crux.Adam(np.float32(LR)))
        b = _buffer(ctx, _data(od, A, B, seed=4))
        info, iq = _iq_step(net, b, B // 2, True, True)
        outs.append((net.get_params(), info, iq))
    assert all(np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32)) for k in range(3))


def test_nan_demo_state_raises_and_leaves_parameters(gpu_ctx):
    ctx, od, A, B = gpu_ctx, 4, 2, 32
    net, _acts = _qnet([od, 64, 64, A], "relu")
    net.attach_optimizer(crux.Adam(np.float32(LR)))
    data = _data(od, A, B); data["s"][2, B - 3] = np.nan          # a demo row
    b = _buffer(ctx, data)
    p0 = net.get_params()
    with pytest.raises(L.CruxError) as e:
        _iq_step(net, b, B // 2, True, False)
    assert e.value.code == L.ENAN and "NaN detected" in str(e.value)
    assert np.array_equal(net.get_params(), p0)


def test_iq_rejects_what_the_reference_cannot_run(gpu_ctx):
    net, _acts = _qnet([4, 16, 2], "relu")
    S = crux.ContinuousSpace(4)
    demo = _buffer(gpu_ctx, _data(4, 2, 16))
    with pytest.raises(ValueError):
        crux.OnlineIQLearn(net, S, demo, N=100, c_opt={"batch_size": 63})
    pi = crux.ActorCritic(crux.GaussianPolicy(parity.chain([4, 8, 1], ["relu", "identity"]), np.zeros(1, np.float32)),
                          crux.DoubleNetwork(crux.ContinuousNetwork(parity.chain([5, 8, 1], ["relu", "identity"])),
                                             crux.ContinuousNetwork(parity.chain([5, 8, 1], ["relu", "identity"]))))
    with pytest.raises(NotImplementedError):
        crux.OnlineIQLearn(pi, S, demo, solver=crux.SAC, N=100)


def test_gradient_penalty_rejects_states_of_the_wrong_width(gpu_ctx):
    """x or xtilde with fewer (or more) rows than the network's input: ValueError before anything reaches the device (the reference: DimensionMismatch)"""
    net, _acts = _qnet([6, 16, 2], "relu")
    x = np.zeros((6, 10), np.float32)
    with pytest.raises(ValueError):
        crux.gradient_penalty(net, np.zeros((4, 10), np.float32))
    with pytest.raises(ValueError):
        crux.gradient_penalty(net, x, np.zeros((7, 10), np.float32))
    with pytest.raises(ValueError):
        crux.gradient_penalty(net, x, np.zeros((6, 9), np.float32))
    assert np.isfinite(crux.gradient_penalty(net, x))


def test_sqil_requires_demo_rewards(gpu_ctx):
    """sqil.jl:31: !haskey(D_demo, :r) && error(...). A device ExperienceBuffer always carries :r, so a demo source without one is a host-side buffer-like object."""
    class NoRewards:
        def haskey(self, k): return k != "r"
    Q, _acts = _qnet([4, 16, 2], "relu")
    with pytest.raises(ValueError, match="reward"):
        crux.SQIL(Q, crux.ContinuousSpace(4), NoRewards(), solver=crux.SoftQ, N=100)


def _fixture_buffer(ctx, name):
    d = dict(np.load(os.path.join(GOLD, name + "_transitions.npz")))
    disc = d["a"].dtype == bool
    A = crux.DiscreteSpace(d["a"].shape[0]) if disc else crux.ContinuousSpace(d["a"].shape[0])
    b = crux.ExperienceBuffer(crux.ContinuousSpace(d["s"].shape[0]), A, d["s"].shape[1], ctx=ctx)
    b.push_({k: d[k] for k in ("s", "a", "sp", "r", "done")}); return b, d


def test_value_training_matches_manual_composition(gpu_ctx):
    """value_training(OnlineIQLearn) over a few iterations == rand!(buffer, demo) -> crux_iq_step -> polyak, composed by hand, bit for bit"""
    ctx, B, epochs, tau, nseed = gpu_ctx, 64, 2, 0.1, 13
    demo, _ = _fixture_buffer(ctx, "cartpole")
    ring = _data(4, 2, 300, seed=8)
    S = crux.ContinuousSpace(4)
    runs = []
    for manual in (False, True):
        net, _acts = _qnet([4, 64, 64, 2], "tanh", seed=3)
        sv = crux.OnlineIQLearn(net, S, demo, N=100, dN=1, c_opt={"batch_size": B, "epochs": epochs, "optimizer": crux.Adam(np.float32(LR))},
                                tau=tau, noise_seed=nseed, buffer_size=300)
        sv.buffer.push_(ring)
        D = crux.buffer_like(sv.buffer, capacity=B)
        infos = []
        for it in range(3):
            sv.i = 10 + it
            if not manual:
                infos.append(crux.value_training(sv, D, np.float32(0.99)))
                continue
            crux.api._ensure_opt(net, sv.c_opt)
            for ep in range(epochs):
                ctr = sv.i * epochs + ep
                crux.rand_(D, sv.buffer, sv.demo, i=sv.i, fracs=[0.5, 0.5], counter=ctr, seed=crux.SAMPLE_SEED)
                _iq_step(net, D, B // 2, True, True, seed=nseed, ctr=ctr)
            crux.polyak_average_(sv.agent.pi_minus, net, tau)
        runs.append((net.get_params(), sv.agent.pi_minus.get_params(), infos))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))
    keys = set(runs[0][2][0])
    assert keys == {"critic_loss", "critic_grad_norm", "softQloss", "valueloss", "avg_R_expert_IQ", "avg_R_demo_IQ", "grad_pen", "reg_loss"}, keys


@pytest.mark.parametrize("algo", ["softq", "sac"])
def test_sqil_zeroes_fresh_rewards_and_draws_half_demo(gpu_ctx, algo):
    ctx, B = gpu_ctx, 32
    if algo == "softq":
        demo, d = _fixture_buffer(ctx, "cartpole")
        mdp = crux.CartPoleMDP(n_envs=1, seed=2)
        Q, _acts = _qnet([4, 32, 32, 2], "relu")
        sv = crux.SQIL(Q, mdp.state_space(), demo, solver=crux.SoftQ, N=400, dN=4, c_opt={"batch_size": B}, buffer_size=500, buffer_init=B, max_steps=50)
    else:
        rng = np.random.default_rng(6); n = 256                                 # (the pendulum fixture records 2 observations; this environment has 3)
        d = {"s": rng.normal(0, 1, (3, n)).astype(np.float32), "a": rng.uniform(-2, 2, (1, n)).astype(np.float32), "sp": rng.normal(0, 1, (3, n)).astype(np.float32),
             "r": rng.uniform(-8, -0.5, (1, n)).astype(np.float32), "done": np.zeros((1, n), bool)}
        demo = crux.ExperienceBuffer(crux.ContinuousSpace(3), crux.ContinuousSpace(1), n, ctx=ctx); demo.push_(d)
        mdp = crux.PendulumMDP(n_envs=1, seed=2)
        pi = crux.ActorCritic(crux.GaussianPolicy(parity.chain([3, 32, 1], ["relu", "identity"]), np.zeros(1, np.float32), seed=1, stream=0),
                              crux.DoubleNetwork(crux.ContinuousNetwork(parity.chain([4, 32, 1], ["relu", "identity"]), seed=1, stream=1),
                                                 crux.ContinuousNetwork(parity.chain([4, 32, 1], ["relu", "identity"]), seed=1, stream=2)))
        sv = crux.SQIL(pi, mdp.state_space(), demo, N=200, dN=20, buffer_init=B, c_opt={"batch_size": B}, a_opt={"batch_size": B}, SAC_alpha_opt={"batch_size": B},
                       buffer_size=500, max_steps=50)
    crux.solve(sv, mdp)
    assert len(sv.history) > 0 and all(np.isfinite(v) for h in sv.history for v in h.values())
    n = len(sv.buffer)
    assert n > 0 and np.all(sv.buffer["r"][:, :n] == 0)                        # sqil_callback on every fresh block
    assert np.array_equal(sv.demo["r"], d["r"])                                 # the demonstrations keep their rewards
    # the last minibatch: B/2 ring rows (reward 0) then B/2 demo rows (the demo's rewards, never 0 in these fixtures)
    r = sv.batch["r"][0]
    assert np.all(r[:B // 2] == 0) and np.all(np.isin(r[B // 2:], d["r"][0])) and np.all(r[B // 2:] != 0)


def test_online_iq_learn_cartpole_beats_random(gpu_ctx):
    """The reference's IQ-Learn CartPole example (examples/il/cartpole.jl: dN=1, c_opt epochs=1, reg=false, gp=false) on the 512 committed demo rows,
    shortened to N=4000. The greedy return of the trained Q against the same network untrained. Observed on MI355X: 190.8 against 9.9."""
    demo, _ = _fixture_buffer(gpu_ctx, "cartpole")
    mdp = crux.CartPoleMDP(n_envs=1, seed=0)
    Q, _acts = _qnet([4, 64, 64, 2], "relu", seed=1)
    sv = crux.OnlineIQLearn(Q, mdp.state_space(), demo, gamma=np.float32(mdp.discount), N=4000, dN=1,
                            c_opt={"epochs": 1, "batch_size": 64, "optimizer": crux.Adam(np.float32(1e-3))}, reg=False, gp=False, max_steps=200, buffer_size=4000)
    crux.solve(sv, mdp)
    greedy = crux.DiscreteNetwork(Q.network, Q.outputs); crux.copyto_(greedy, Q)
    ret = crux.undiscounted_return(crux.Sampler(crux.CartPoleMDP(n_envs=1, seed=5), greedy, max_steps=200), Neps=20)
    untrained, _ = _qnet([4, 64, 64, 2], "relu", seed=1)
    rnd = crux.undiscounted_return(crux.Sampler(crux.CartPoleMDP(n_envs=1, seed=5), untrained, max_steps=200), Neps=20)
    print("iq cartpole: greedy return %.1f, untrained %.1f" % (ret, rnd))
    assert ret > 100.0 and ret > 5 * rnd, (ret, rnd)
