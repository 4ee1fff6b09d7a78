"""Float64 yardstick of the DiagonalFisherRegularizer (src/extras/fisher_information.jl), written from its formulas:

    R          = lam / A * sum_a mean_a(F .* (theta - theta_prev)^2)              every parameter array's mean with its own divisor
    dR/dtheta  = 2 lam / (A numel_a) * F_i (theta_i - theta_prev_i)               F and theta_prev constant
    add        : N += 1; F += (g .* g - F) / N

over the array table of a Chain(Dense...) handle in the flat Flux.params layout: W_0, b_0, ..., W_{L-1}, b_{L-1}, then the trailing extras as ONE array.
`value_f32` / `gradient_f32` restate the device's arithmetic (Float32 terms, Float64 accumulation, csrc/fisher.hip); `add_f32` is numpy's Float32 running mean, the
expression the device is bitwise equal to. tests/test_fisher_reference.py pins the yardstick against torch autograd in float64."""
import numpy as np


def array_table(dims, n_extra=0):
    """[(offset, length)] of the parameter arrays of a handle with layer widths `dims` and `n_extra` trailing extras"""
    tab, off = [], 0
    for l in range(len(dims) - 1):
        for n in (dims[l] * dims[l + 1], dims[l + 1]):
            tab.append((off, n)); off += n
    if n_extra > 0:
        tab.append((off, n_extra)); off += n_extra
    return tab


def n_params(dims, n_extra=0):
    return sum(n for _, n in array_table(dims, n_extra))


def value(theta, theta_prev, F, lam, table):
    th, pv, F = (np.asarray(a, np.float64) for a in (theta, theta_prev, F))
    tot = 0.0
    for off, n in table:
        s = slice(off, off + n)
        tot += float(np.mean(F[s] * (th[s] - pv[s]) ** 2))
    return float(lam) * tot / len(table)


def gradient(theta, theta_prev, F, lam, table):
    th, pv, F = (np.asarray(a, np.float64) for a in (theta, theta_prev, F))
    g = np.zeros_like(th)
    for off, n in table:
        s = slice(off, off + n)
        g[s] = 2.0 * float(lam) / (len(table) * n) * F[s] * (th[s] - pv[s])
    return g


def add(F, g, N):
    """one add_fisher_information_diagonal! in float64: returns (F', N + 1)"""
    F, g = np.asarray(F, np.float64), np.asarray(g, np.float64)
    return F + (g * g - F) / float(N + 1), N + 1


def add_f32(F, g, N0, times=1):
    """`times` adds with one gradient in numpy float32 -- the device's definition, bit for bit"""
    F, g = np.asarray(F, np.float32).copy(), np.asarray(g, np.float32)
    for t in range(1, times + 1):
        F = (F + (g * g - F) / np.float32(N0 + t)).astype(np.float32)
    return F


def value_f32(theta, theta_prev, F, lam, table):
    th, pv, F = (np.asarray(a, np.float32) for a in (theta, theta_prev, F))
    tot = 0.0
    for off, n in table:
        s = slice(off, off + n)
        d = (th[s] - pv[s]).astype(np.float32); t = ((F[s] * d).astype(np.float32) * d).astype(np.float32)
        tot += float(np.sum(t.astype(np.float64) / float(n)))
    return float(np.float32(float(np.float32(lam)) / len(table) * tot))


def gradient_f32(theta, theta_prev, F, lam, table):
    th, pv, F = (np.asarray(a, np.float32) for a in (theta, theta_prev, F))
    g = np.zeros_like(th)
    for off, n in table:
        s = slice(off, off + n)
        c = np.float32(2.0 * float(np.float32(lam)) / (len(table) * n))
        d = (th[s] - pv[s]).astype(np.float32)
        g[s] = (c * (F[s] * d).astype(np.float32)).astype(np.float32)
    return g


def draw(rng, dims, n_extra):
    """the inputs the tests use: theta of order 0.5, theta - theta_prev of order 0.1, F squares of standard normals"""
    n = n_params(dims, n_extra)
    theta = (0.5 * rng.standard_normal(n)).astype(np.float32)
    prev = (theta + 0.1 * rng.standard_normal(n)).astype(np.float32)
    F = (rng.standard_normal(n) ** 2).astype(np.float32)
    return theta, prev, F
