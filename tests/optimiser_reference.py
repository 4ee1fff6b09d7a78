"""Host-only reference of Flux.Optimiser(ClipValue(c), Adam(eta, (b1, b2), eps)) as csrc/sac.hip applies it (AdamClipGatedOp).

  clip_value          the element rule g > c ? c : g < -c ? -c : g (clamp! inside apply!(::ClipValue)); a NaN passes unchanged, as in the kernel
  chain_steps_f64     k steps in float64: parameters, moments and beta powers after every step (THE reference; tests/test_optimiser_reference.py pins it against
                      torch.nn.utils.clip_grad_value_ + torch.optim.Adam in float64)
  first_step_mv_f32   m and v after the first step from zero moments, exactly as the kernel's Float64 expressions round them to Float32
  teacher_forced_f64  one step in float64 from a given Float32 state (p, m, v), gradient and step number t: what the device's next state is compared with
  moment_bounds       |m| <= (1 - b1^t) c and v <= (1 - b2^t) c^2 after t clamped steps from zero moments
"""
import numpy as np

B1, B2, EPS = 0.9, 0.999, 1e-8


def clip_value(g, c):
    g = np.asarray(g)
    c = g.dtype.type(c)
    return np.where(g > c, c, np.where(g < -c, -c, g)).astype(g.dtype)


def chain_steps_f64(p, grads, c, eta, b1=B1, b2=B2, eps=EPS):
    """grads: one gradient per step. Returns [(p, m, v)] after every step, float64. c = None or 0: plain Adam."""
    p = np.asarray(p, np.float64).copy(); m, v = np.zeros_like(p), np.zeros_like(p); bp1, bp2 = b1, b2; out = []
    for g in grads:
        g = np.asarray(g, np.float64)
        if c:
            g = clip_value(g, c)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + ((1.0 - b2) * g) * g
        p = p - m / (1.0 - bp1) / (np.sqrt(v / (1.0 - bp2)) + eps) * eta
        bp1 *= b1; bp2 *= b2
        out.append((p.copy(), m.copy(), v.copy()))
    return out


def first_step_mv_f32(g, c, b1=B1, b2=B2):
    """(float)(b1 * 0 + (1 - b1) * gd), (float)(b2 * 0 + ((1 - b2) * gd) * gd) with gd = (double)clip_value(g, c): bit for bit what AdamClipGatedOp stores"""
    gd = clip_value(np.asarray(g, np.float32), c).astype(np.float64) if c else np.asarray(g, np.float32).astype(np.float64)
    return ((1.0 - b1) * gd).astype(np.float32), (((1.0 - b2) * gd) * gd).astype(np.float32)


def teacher_forced_f64(p, m, v, g, t, c, eta, b1=B1, b2=B2, eps=EPS):
    """step number t (1-based) from the Float32 state (p, m, v) and the raw Float32 gradient g, everything in float64: returns (p' - p, m', v')"""
    gd = np.asarray(g, np.float32).astype(np.float64)
    if c:
        gd = clip_value(gd, np.float64(np.float32(c)))
    m1 = b1 * np.asarray(m, np.float64) + (1.0 - b1) * gd
    v1 = b2 * np.asarray(v, np.float64) + ((1.0 - b2) * gd) * gd
    return -(m1 / (1.0 - b1 ** t) / (np.sqrt(v1 / (1.0 - b2 ** t)) + eps) * eta), m1, v1


def ulp32(x):
    """the Float32 spacing at |x| (at least the smallest normal's)"""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float64)), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def moment_bounds(t, c, b1=B1, b2=B2):
    """after t steps from zero moments every clamped gradient has |g| <= c: |m| <= (1 - b1^t) c, v <= (1 - b2^t) c^2 (geometric sums); + one Float32 rounding per step"""
    slack = 1.0 + 2.0 * t * 2.0 ** -24
    return (1.0 - b1 ** t) * c * slack, (1.0 - b2 ** t) * c * c * slack
