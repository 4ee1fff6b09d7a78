"""CPU tests of tests/optimiser_reference.py and of the host classes ClipValue / Optimiser / refuse_optimiser_chain. No GPU, no library call."""
import numpy as np
import pytest

import optimiser_reference as OR


def test_clip_value_is_the_kernels_element_rule():
    g = np.array([-3.0, -1.0, -0.5, 0.0, 0.5, 1.0, 3.0, np.nan, np.inf, -np.inf], np.float32)
    out = OR.clip_value(g, 1.0)
    assert out.dtype == np.float32 and np.array_equal(out[:7], [-1.0, -1.0, -0.5, 0.0, 0.5, 1.0, 1.0]) and np.isnan(out[7]) and out[8] == 1.0 and out[9] == -1.0


@pytest.mark.parametrize("c", [0.05, 1.0])
def test_chain_is_torch_clip_grad_value_then_adam_in_float64(c):
    import torch
    torch.set_num_threads(1)
    rng = np.random.default_rng(7); n, eta = 257, 1e-3
    p0 = rng.normal(0, 1, n); grads = [rng.normal(0, 3 * c, n) for _ in range(3)]
    ref = OR.chain_steps_f64(p0, grads, c, eta)
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True); opt = torch.optim.Adam([pt], lr=eta, betas=(OR.B1, OR.B2), eps=OR.EPS)
    for t, g in enumerate(grads):
        pt.grad = torch.tensor(g, dtype=torch.float64)
        torch.nn.utils.clip_grad_value_([pt], c)
        opt.step()
        st = opt.state[pt]; p, m, v = ref[t]
        for name, a, b in (("p", p, pt.detach().numpy()), ("m", m, st["exp_avg"].numpy()), ("v", v, st["exp_avg_sq"].numpy())):
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (t, name, float(np.abs(a - b).max()))
    assert 0.3 < np.mean(np.abs(grads[0]) > c) < 0.9      # the clamp was at work
    plain = OR.chain_steps_f64(p0, grads, None, eta)
    assert np.abs(plain[0][1] - ref[0][1]).max() > 0       # and it changes the moments


def test_first_step_moments_round_as_the_kernel_does():
    rng = np.random.default_rng(8); g = rng.normal(0, 2, 1000).astype(np.float32); c = np.float32(0.7)
    m, v = OR.first_step_mv_f32(g, c)
    gc = np.clip(g, -c, c)
    assert m.dtype == np.float32 and v.dtype == np.float32
    for i in range(0, 1000, 37):      # the scalar restatement of AdamClipGatedOp's two expressions
        gd = float(gc[i])
        assert m[i] == np.float32(0.9 * 0.0 + (1.0 - 0.9) * gd) and v[i] == np.float32(0.999 * 0.0 + ((1.0 - 0.999) * gd) * gd)
    bm, bv = OR.moment_bounds(1, float(c))
    assert np.abs(m).max() <= bm and v.max() <= bv
    m0, v0 = OR.first_step_mv_f32(g, 0)
    assert np.abs(m0).max() > bm and v0.max() > bv      # the unclamped twin violates them
    d, m64, v64 = OR.teacher_forced_f64(np.zeros(1000, np.float32), np.zeros(1000, np.float32), np.zeros(1000, np.float32), g, 1, c, 1e-3)
    assert np.all(np.abs(m - m64) <= OR.ulp32(m64)) and np.all(np.abs(v - v64) <= OR.ulp32(v64)) and np.abs(d).max() <= 1e-3 * (1 + 1e-6)


def test_host_classes_validate():
    import crux_jl_amd as crux
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            crux.ClipValue(bad)
    a = crux.Adam(np.float32(1e-3)); o = crux.Optimiser(crux.ClipValue(np.float32(1)), a)
    assert (o.eta, o.beta, o.epsilon) == (a.eta, a.beta, a.epsilon) and o.clip.thresh == 1.0
    lone = crux.Optimiser(a)
    assert lone.clip is None and lone.eta == a.eta
    for parts, name in (((crux.ClipValue(1.0),), "ClipValue"), ((a, crux.ClipValue(1.0)), "Adam, ClipValue"), ((crux.ClipValue(1.0), crux.ClipValue(2.0), a), "ClipValue, ClipValue, Adam"),
                        ((a, a), "Adam, Adam"), ((), "Optimiser()")):
        with pytest.raises(NotImplementedError) as e:
            crux.Optimiser(*parts)
        assert name in str(e.value)
    crux.refuse_optimiser_chain(a, "x"); crux.refuse_optimiser_chain(lone, "x")      # no clamp: passes
    with pytest.raises(NotImplementedError) as e:
        crux.refuse_optimiser_chain(o, "some learner")
    assert "some learner" in str(e.value) and "ClipValue" in str(e.value)
