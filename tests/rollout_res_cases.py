"""Cases of the register-resident WIDE rollout kernel k_rollout_res<H> (csrc/env.hip: 8 -> H -> H -> 4 on the synthetic discrete environment, 3 -> H -> H -> 1 on Pendulum,
H = 128 or 256) on every head, activation, ring edge and episode edge it serves, with NON-ZERO biases.

Host only: nothing here needs a device until Case.gpu_policy() / gpu_sampler() / gpu_buffer() are called (tests/test_rollout_res_cases.py uses the oracle alone).

  CASES / EVAL_CASES     the table: one Case per name (fields below); EVAL_CASES are the greedy policies of the batched evaluation (crux.episodes_)
  takes_res(case, T)     the dispatch condition of crux_rollout restated: three layers, equal hidden widths in {128, 256}, T >= 2, Pendulum 3/1/1 or synth-discrete 8/4/4,
                         no two-headed handle (no case here has one)
  Case.params()          Glorot's draws (the same Philox draws on both sides) + N(0, PARAM_NOISE) on EVERY parameter: Glorot leaves b1 / b2 / b3 at zero, and a wrong bias lane
                         passes every test whose biases are zero
  Case.rows()            where every transition of the call sequence lands: ring row, environment, call, step, the sampler's draw counter and the interaction counter
  oracle_run(case)       the oracle's trajectory of the whole call sequence (optionally with every parameter multiplied by 1 + 1e-5 n: the decision-margin runs)

A block of a call is env-major: environment e owns the rows (base + e T + t) % capacity (sampler.jl:139-173 for a Vector of Samplers), so a ring whose end falls inside a block
is crossed either inside one environment's rows or between two environments' rows, depending on where the block starts; `fill` rows pushed from the host put it there."""
import ctypes as C

import numpy as np

import oracle as O
from crux_jl_amd import _lib as L

SYNTH, PEND = "synth_discrete", "pendulum"
RELU3, TANH_OUT, TANH_HID = ["relu", "relu", "identity"], ["relu", "relu", "tanh"], ["tanh", "tanh", "identity"]
PARAM_NOISE = 0.05
LOGSIGMA0 = -0.4
ASCALE = 2.0
JITTER = 1e-5             # the decision-margin runs multiply every parameter by 1 + JITTER n, n ~ N(0, 1)
DISCRETE_HEADS = ("eps_greedy", "categorical", "softq", "greedy", "always_stochastic")
EXPLORING = ("eps_greedy", "categorical", "softq", "gaussian", "squashed", "noise")      # steps!(...; explore = true); the others are action(pi, s)
NOISE = {"sigma": 0.3, "eps_min": -0.3, "eps_max": 0.3, "a_min": -0.4, "a_max": 0.4}     # GaussianNoiseExplorationPolicy: all four clamps finite
F, T_ = False, True


class Case:
    def __init__(self, name, env, H, head, acts=RELU3, E=1, calls=((4, F),), cap=None, fill=0, max_steps=100, whiten=False, extras=(), prioritized=False,
                 eps=(1.0, 0.05, 8), i0=0, seeds=None, events=(), seam=False):
        self.name, self.env, self.H, self.head, self.acts, self.E = name, env, H, head, list(acts), E
        self.calls = [(int(t), bool(r)) for t, r in calls]
        self.n_rows = E * sum(t for t, _ in self.calls)
        self.cap, self.fill, self.max_steps = cap or self.n_rows, fill, max_steps
        self.mu, self.sigma = (0.01, 0.5) if whiten else (0.0, 1.0)      # the values of test_synthetic_env_rollout_matches_oracle
        self.extras, self.prioritized, self.eps, self.i0 = list(extras), prioritized, eps, i0
        self.events, self.seam = set(events), seam
        self.od, self.ad = (8, 4) if env == SYNTH else (3, 1)
        self.dims = [self.od, H, H, self.ad]
        self.disc = head in DISCRETE_HEADS
        self.n_extra = self.ad if head in ("gaussian", "squashed") else 0
        self.explore = head in EXPLORING
        self.two_headed = False
        self.net_seed, self.env_seed, self.noise_seed = seeds

    def __repr__(self):
        return self.name

    # ---- the policy ------------------------------------------------------------------------------------------------------------------
    def _glorot(self):
        o = O.OMlp(self.dims, self.acts, self.n_extra).init_glorot(self.net_seed, 0, LOGSIGMA0)
        if self.head == "squashed":
            O.chk(O.lib().orc_mlp_set_squash(o.h, ASCALE))
        return o

    def params(self, jitter_seed=None):
        o = self._glorot(); p0 = o.params.copy()      # (o.params is a view of the oracle's memory: o stays alive until the copy exists)
        p = p0 + np.random.default_rng(self.noise_seed).normal(0.0, PARAM_NOISE, p0.size).astype(np.float32)
        if jitter_seed is not None:
            p = (p * (1.0 + JITTER * np.random.default_rng(jitter_seed).standard_normal(p.size))).astype(np.float32)
        return p

    def oracle_policy(self, jitter_seed=None):
        o = self._glorot(); o.params[:] = self.params(jitter_seed)
        return o

    def gpu_policy(self):
        """the device twin: the same Glorot draws (asserted), then the same noised parameters"""
        import crux_jl_amd as crux
        import parity
        ch, kw = parity.chain(self.dims, self.acts), {"seed": self.net_seed, "stream": 0}
        if self.disc:
            g = crux.DiscreteNetwork(ch, list(range(1, self.ad + 1)), always_stochastic=self.head == "always_stochastic", **kw)
            if self.head == "softq":
                g.logit_div = 0.5
        elif self.head == "gaussian":
            g = crux.GaussianPolicy(ch, np.full(self.ad, LOGSIGMA0, np.float32), **kw)
        elif self.head == "squashed":
            g = crux.SquashedGaussianPolicy(ch, np.full(self.ad, LOGSIGMA0, np.float32), ascale=ASCALE, **kw)
        else:
            g = crux.ContinuousNetwork(ch, **kw)
        o = self._glorot()
        assert np.array_equal(g.get_params(), o.params)
        g.set_params(self.params())
        return g

    def gpu_sampler(self, g, n_envs=None):
        import crux_jl_amd as crux
        pe = None
        if self.head == "eps_greedy":
            pe = crux.EpsGreedyPolicy(crux.LinearDecaySchedule(*self.eps), list(range(1, self.ad + 1)))
        elif self.head == "noise":
            pe = crux.GaussianNoiseExplorationPolicy(**NOISE)
        mdp = crux.GymMDP(self.env, n_envs=n_envs or self.E, seed=self.env_seed, obs_dim=self.od, act_dim=self.ad)
        S = crux.ContinuousSpace(self.od, mu=np.full(self.od, self.mu, np.float32), sigma=np.full(self.od, self.sigma, np.float32))
        return crux.Sampler(mdp, crux.PolicyParams(g, pi_explore=pe), S=S, max_steps=self.max_steps, required_columns=self.extras)

    def gpu_buffer(self):
        import crux_jl_amd as crux
        A = crux.DiscreteSpace(self.ad) if self.disc else crux.ContinuousSpace(self.ad)
        b = crux.ExperienceBuffer(crux.ContinuousSpace(self.od), A, self.cap, self.extras, prioritized=self.prioritized)
        for d in self.fill_blocks():
            b.push_(d)
        if self.prioritized:
            ids0, v = self.fill_priorities()
            b.update_priorities_(ids0 + 1, v)
            b.cumsum()      # the tree is whole before the first rollout: the in-kernel push bodies update it in place
        return b

    # ---- the oracle's side -----------------------------------------------------------------------------------------------------------
    def cfg(self, reset, i):
        """crux_rollout_cfg of one steps! call, written from the case (core._rollout_cfg derives its own from the policy objects)"""
        head = {"eps_greedy": "greedy_q", "categorical": "categorical", "softq": "categorical", "greedy": "categorical", "always_stochastic": "categorical",
                "gaussian": "gaussian", "squashed": "gaussian", "noise": "deterministic", "deterministic": "deterministic"}[self.head]
        cfg = L.RolloutCfg()
        cfg.explore, cfg.reset_at_end, cfg.head, cfg.i0 = (2 if self.head == "always_stochastic" else int(self.explore)), int(reset), L.HEAD[head], int(i)
        cfg.eps_steps, cfg.noise_sigma, cfg.logit_div = 0, -1.0, 0.5 if self.head == "softq" else 0.0
        cfg.noise_eps_min, cfg.noise_eps_max, cfg.a_min, cfg.a_max = -np.inf, np.inf, -np.inf, np.inf
        if self.head == "eps_greedy":
            cfg.eps_start, cfg.eps_stop, cfg.eps_steps = self.eps
        if self.head == "noise":
            cfg.noise_sigma, cfg.noise_eps_min, cfg.noise_eps_max, cfg.a_min, cfg.a_max = NOISE["sigma"], NOISE["eps_min"], NOISE["eps_max"], NOISE["a_min"], NOISE["a_max"]
        return cfg

    def oracle_env(self, n_envs=None):
        return O.OEnv(self.env, n_envs or self.E, self.max_steps, 0.99, self.env_seed, mu=np.full(self.od, self.mu, np.float32), sigma=np.full(self.od, self.sigma, np.float32),
                      so=self.od, sa=self.ad)

    def oracle_buffer(self, extras=None):
        extras = list(self.extras if extras is None else extras)
        if self.prioritized and "weight" not in extras:
            extras.append("weight")      # a prioritized buffer has the column (experience_buffer.jl:71)
        ob = O.OBuffer(self.od, self.ad, L.ACTION_DISCRETE if self.disc else L.ACTION_CONTINUOUS, self.cap, extras, prioritized=self.prioritized, alpha=np.float32(0.6))
        for d in self.fill_blocks():
            ob.push(d)
        if self.prioritized:
            ids0, v = self.fill_priorities()
            O.chk(O.lib().orc_per_update(ob.h, O.vpz(ids0), O.vpz(v), 0, ids0.size))
        return ob

    # ---- the ring before the first call ----------------------------------------------------------------------------------------------
    def fill_blocks(self):
        """`fill` rows pushed from the host before the first call, at most a capacity per push: they move the start row (and fill a prioritized ring)"""
        rng, out, left = np.random.default_rng(self.noise_seed + 1), [], self.fill
        while left > 0:
            n = min(left, self.cap); left -= n
            a = np.eye(self.ad, dtype=bool)[:, rng.integers(0, self.ad, n)] if self.disc else rng.normal(0, 1, (self.ad, n)).astype(np.float32)
            d = {"s": rng.normal(0, 1, (self.od, n)).astype(np.float32), "a": a, "sp": rng.normal(0, 1, (self.od, n)).astype(np.float32),
                 "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": rng.random((1, n)) < 0.1, "episode_end": rng.random((1, n)) < 0.2}
            for k in self.extras:
                d[k] = rng.integers(1, 50, (1, n)).astype(np.int64) if k in ("t", "i") else rng.normal(0, 1, (1, n)).astype(np.float32)
            out.append(d)
        return out

    def fill_priorities(self):
        """update_priorities! on every row of the full ring: the priorities the pushes meet are all different"""
        rng = np.random.default_rng(self.noise_seed + 2)
        return np.arange(self.cap, dtype=np.int64), (np.abs(rng.standard_normal(self.cap)) + 0.05).astype(np.float32)

    def rows(self):
        """one entry per transition, call by call and env-major inside a call: dict of int64 arrays
        j ring row, e environment, call, t step of the call, ctr steps environment e had taken before (the Philox counter of its draws), gi the interaction counter i + t E + e"""
        out = {k: [] for k in ("j", "e", "call", "t", "ctr", "gi", "T")}
        base, i, taken = self.fill % self.cap, self.i0, 0
        for c, (T, _) in enumerate(self.calls):
            for e in range(self.E):
                for t in range(T):
                    for k, v in (("j", (base + e * T + t) % self.cap), ("e", e), ("call", c), ("t", t), ("ctr", taken + t), ("gi", i + t * self.E + e), ("T", T)):
                        out[k].append(v)
            base = (base + self.E * T) % self.cap; i += self.E * T; taken += T
        return {k: np.asarray(v, np.int64) for k, v in out.items()}


def takes_res(case, T):
    d = case.dims
    shape = (case.env == PEND and d[0] == 3 and d[-1] == 1 and case.ad == 1) or (case.env == SYNTH and d[0] == 8 and d[-1] == 4 and case.ad == 4)
    return len(d) == 4 and d[1] == d[2] and d[1] in (128, 256) and T >= 2 and shape and not case.two_headed


class Run:
    """what one pass over a case's call sequence left behind"""

    def __init__(self, cols, state, per_call):
        self.cols, self.state, self.per_call = cols, state, per_call      # per_call: [(sum_r, n_episode_end, next_ind 1-based)]


def oracle_run(case, jitter_seed=None, extras=None):
    o, ob, oe = case.oracle_policy(jitter_seed), case.oracle_buffer(extras), case.oracle_env()
    i, per_call = case.i0, []
    for T, reset in case.calls:
        sr, ne = oe.rollout(o, case.cfg(reset, i), ob, T)
        per_call.append((sr, ne, int(O.lib().orc_buffer_next_ind(ob.h)) + 1)); i += case.E * T
    run = Run({k: ob[k] for k in ob.keys()}, oe.state(), per_call)
    run.policy = o
    if case.prioritized:
        pr = np.empty(case.cap, np.float32); mx, mn = C.c_float(), C.c_float()
        O.chk(O.lib().orc_per_get(ob.h, O.vpz(pr), C.byref(mx), C.byref(mn), None)); run.priorities = (pr, mx.value, mn.value)
    return run


_ORACLE = {}


def oracle_reference(case):
    """the oracle's run of a case, computed once per process and shared (callers do not write into it)"""
    if case.name not in _ORACLE:
        _ORACLE[case.name] = oracle_run(case)
    return _ORACLE[case.name]


def philox_u64(seed, ctr, stream, purpose):
    """the Float64 uniform the heads compare with eps: words 0 and 1 of crux_philox(seed, ctr, stream, purpose) (include/crux_rng.h)"""
    v = np.empty(4, np.uint32); O.lib().orc_philox(int(seed), int(ctr), int(stream), int(purpose), O.vpz(v))
    return float(((int(v[0]) << 32 | int(v[1])) >> 11) * 2.0 ** -53)


# ---- the table -------------------------------------------------------------------------------------------------------------------------
# geometry, spread over the heads (E in {1, 3}; T in {1, 2, 3, 4, 33}; at most 38 steps per environment):
C3 = [(4, F)] * 3                          # three DN = 4 calls of an off-policy solve on one sampler
MIXED = [(1, F), (3, F), (1, F), (4, F)]   # T = 1 goes to the generic kernel, T >= 2 to the resident one: the two alternate on one sampler state
# E = 3, T = 4, capacity 37: the second block starts at fill + 12 and crosses the ring end ...
WRAP_IN = {"E": 3, "calls": C3, "cap": 37, "fill": 23, "events": ["wrap_inside_env0"]}            # ... after two rows of environment 0 (rows 35, 36, 0, 1)
WRAP_BETWEEN = {"E": 3, "calls": C3, "cap": 37, "fill": 21, "events": ["wrap_between_envs"]}      # ... exactly between environment 0 (rows 33 .. 36) and environment 1 (0 .. 3)
# max_steps = 5: the first launch leaves an episode of 2 steps open, the second ends it by max_steps on its LAST step, the third holds six more ends by max_steps
ENDS = {"max_steps": 5, "events": ["max_steps_end", "end_on_last_step"]}
ENDS_NORESET = dict(ENDS, calls=[(2, F), (3, F), (33, F)])
ENDS_RESET = dict(ENDS, calls=[(2, F), (3, T_), (33, T_)])      # with reset_at_end: the end on the last step must not be counted twice, the 33-step launch ends 3 steps into an episode
ALLCOLS = ["t", "i", "weight", "cost"]
LP = ["logprob"]

_TEMPLATES = [
    # name, env, head, {H: keyword arguments}
    ("eps_greedy", SYNTH, "eps_greedy", {256: dict(calls=C3, extras=LP), 128: dict(E=3, calls=MIXED, extras=LP, eps=(1.0, 0.05, 20))}),
    ("categorical", SYNTH, "categorical", {256: dict(WRAP_IN, extras=LP, seam=True), 128: dict(WRAP_BETWEEN, extras=LP, seam=True, whiten=True)}),
    ("softq", SYNTH, "softq", {256: dict(calls=[(33, F)], extras=LP), 128: dict(calls=[(2, F)], extras=LP)}),
    ("greedy", SYNTH, "greedy", {256: dict(calls=[(3, F)], extras=ALLCOLS), 128: dict(E=3, calls=[(33, F)])}),
    # (logprob is NaN by definition here and the dynamics are driven by the action index alone: the draws are all that shows the logits, so these two cases are long)
    ("always_stochastic", SYNTH, "always_stochastic", {256: dict(E=3, calls=[(33, T_)], extras=LP), 128: dict(E=3, calls=[(33, F)], extras=LP)}),
    ("gaussian", PEND, "gaussian", {256: dict(WRAP_BETWEEN, extras=LP, seam=True, whiten=True), 128: dict(WRAP_IN, extras=LP, seam=True)}),
    ("squashed", PEND, "squashed", {256: dict(calls=[(33, T_)], extras=LP), 128: dict(E=3, calls=[(3, F)], extras=LP)}),
    ("noise", PEND, "noise", {256: dict(calls=C3, extras=ALLCOLS), 128: dict(E=3, calls=[(33, F)])}),
    ("noise_tanh_out", PEND, "noise", {256: dict(calls=[(33, F)], acts=TANH_OUT), 128: dict(E=3, calls=MIXED, acts=TANH_OUT)}),
    ("gaussian_tanh_hidden", PEND, "gaussian", {256: dict(calls=C3, extras=LP, acts=TANH_HID), 128: dict(E=3, calls=[(2, F)], extras=LP, acts=TANH_HID)}),
    ("ends_noreset", None, None, {256: dict(ENDS_NORESET, env=SYNTH, head="categorical", E=3, extras=["t", "logprob"]),
                                  128: dict(ENDS_NORESET, env=PEND, head="gaussian", extras=["t", "logprob"])}),
    ("ends_reset", None, None, {256: dict(ENDS_RESET, env=PEND, head="squashed", E=3, extras=["t", "logprob"]),
                                128: dict(ENDS_RESET, env=SYNTH, head="eps_greedy", extras=["t", "logprob"], eps=(1.0, 0.05, 20))}),
    # a full prioritized ring of 129 rows, the start row at 100: push!'s bookkeeping runs inside the rollout launch (one environment), push_touch_small for the 4 rows,
    # push_touch_block for the 33, which also cross the ring end
    ("prioritized", SYNTH, "eps_greedy", {256: dict(calls=[(4, F), (33, F)], cap=129, fill=229, prioritized=True, eps=(1.0, 0.05, 20), events=["wrap_inside_env0"])}),
]
# (case name) -> (network seed, environment seed, parameter-noise seed) where the default draw misses a condition of tests/test_rollout_res_cases.py (a case that misses gets
# other seeds; none may be dropped)
SEED_OVERRIDES = {"always_stochastic_h128": (1109, 1209, 1309),      # the default draw left b3[3] at -0.0019
                  "squashed_h256": (1112, 1212, 1312)}               # the default draw left b3 at -0.0006


def _build(templates, start=0):
    out = []
    for n, (name, env, head, per_h) in enumerate(templates):
        for H in sorted(per_h, reverse=True):
            kw = dict(per_h[H]); full = "%s_h%d" % (name, H); k = start + 2 * n + (H == 128)
            out.append(Case(full, kw.pop("env", env), H, kw.pop("head", head), seeds=SEED_OVERRIDES.get(full, (100 + k, 200 + k, 300 + k)), **kw))
    return out


CASES = _build(_TEMPLATES)
# crux.episodes_ with Neps = 3 and max_steps = 12: one launch of E = 3 fresh environments, T = 12, reset at its end
_EVAL = dict(E=3, calls=[(12, T_)], max_steps=12)
EVAL_CASES = _build([("eval_greedy", SYNTH, "greedy", {256: _EVAL, 128: _EVAL}), ("eval_deterministic", PEND, "deterministic", {256: _EVAL, 128: _EVAL})], start=60)
