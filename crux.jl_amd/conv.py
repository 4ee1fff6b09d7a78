"""conv.py -- convolutional layers in a Chain and the trunk of a conv policy (csrc/conv.hip; examples/rl/atari.jl of the reference).

    Chain(Scale(1 / 255), Conv((8, 8), 4, 16, "relu", stride=4), Conv((4, 4), 16, 32, "relu", stride=2), flatten, Dense(2048, 256, "relu"), Dense(256, n), input=(80, 80, 4))

A chain that starts with `[Scale,] Conv+, flatten` is split into a trunk (a crux_conv descriptor plus a bare-vector parameter handle) and the dense head that follows; a
DiscreteNetwork / ContinuousNetwork over such a chain keeps the head in `.head_h` / `.network.dims` and the trunk in `.trunk`; its `.h` raises (core.NetworkPolicy.h: there is
no handle of the whole network, and code that reads one would run the head over raw observations). Semantics are Flux's: WHCN column-major
images (a flattened observation has index w + W (h + H c)), (k1, k2, cin, cout) weights, a true (flipped) convolution, flatten in WHC order.

What takes a conv policy: value / forward, the parameter and optimiser accessors (trunk first, then head: Flux.params order), polyak_average_, copyto_, clone_policy,
policy_explore on the host seam (a HostMDP: pixel environments live on the host), and DQN through solve. Everything else refuses it by name (core.refuse_conv)."""
import ctypes as C

import numpy as np

from . import _lib as L
from .core import Dense, ParamVector, _vp, default_context


def _two(v, what):
    t = (int(v), int(v)) if isinstance(v, (int, np.integer)) else tuple(int(q) for q in v)
    if len(t) != 2:
        raise ValueError("Conv: %s must be an integer or a pair, got %r" % (what, v))
    return t


class Conv:
    """Flux.Conv((k1, k2), cin => cout, act; stride, pad): pad symmetric per axis. dilation and groups other than 1 are not implemented."""
    conv_kind = "conv"

    def __init__(self, k, cin, cout, act="identity", stride=1, pad=0, dilation=1, groups=1):
        self.k, self.cin, self.cout = _two(k, "the kernel size"), int(cin), int(cout)
        self.act = act if isinstance(act, str) else getattr(act, "__name__", "identity")
        self.stride, self.pad, self.dilation, self.groups = _two(stride, "stride"), _two(pad, "pad"), _two(dilation, "dilation"), int(groups)
        if self.dilation != (1, 1):
            raise NotImplementedError("Conv: dilation = %r is not implemented (dilation 1 only)" % (dilation,))
        if self.groups != 1:
            raise NotImplementedError("Conv: groups = %d is not implemented (groups 1 only)" % self.groups)
        if self.act not in L.ACT:
            raise ValueError("Conv: activation %r, one of %s" % (self.act, sorted(L.ACT)))


class _Flatten:
    """Flux.flatten: [OW, OH, cout, B] -> [OW OH cout, B]"""
    conv_kind = "flatten"


flatten = _Flatten()


class Scale:
    """x -> c * x as the first layer of a conv chain (the `x ./ 255f0` prelude, with c = 1 / 255): one Float32 multiply folded into the first layer's operand load"""
    conv_kind = "scale"

    def __init__(self, c):
        self.c = float(np.float32(c))


class ConvSpec:
    """the trunk of a chain: input extent, input scale, the Conv layers, and the extents between them"""

    def __init__(self, W, H, C_, scale, convs):
        self.W, self.H, self.C, self.scale, self.convs = int(W), int(H), int(C_), float(scale), list(convs)
        self.extents = [(self.W, self.H, self.C)]
        for n, l in enumerate(self.convs):
            w, h, c = self.extents[-1]
            if l.cin != c:
                raise ValueError("Chain: Conv layer %d takes %d channels, its input has %d" % (n, l.cin, c))
            ow, oh = (w + 2 * l.pad[0] - l.k[0]) // l.stride[0] + 1, (h + 2 * l.pad[1] - l.k[1]) // l.stride[1] + 1
            if l.k[0] > w + 2 * l.pad[0] or l.k[1] > h + 2 * l.pad[1] or ow < 1 or oh < 1:
                raise ValueError("Chain: Conv layer %d (%d x %d) does not fit its %d x %d input with pad %r" % (n, l.k[0], l.k[1], w, h, l.pad))
            self.extents.append((ow, oh, l.cout))

    @property
    def in_features(self):
        return self.W * self.H * self.C

    @property
    def out_features(self):
        w, h, c = self.extents[-1]
        return w * h * c

    @property
    def shapes(self):
        """Flux.params of the trunk: [(k1, k2, cin, cout), (cout,), ...]"""
        out = []
        for l in self.convs:
            out += [l.k + (l.cin, l.cout), (l.cout,)]
        return out

    @property
    def n_params(self):
        return sum(int(np.prod(s)) for s in self.shapes)


def split_chain(layers, input):
    """[Scale,] Conv+, flatten, Dense+ -> (ConvSpec, the Dense layers), shapes checked against the input extent (W, H, C)"""
    layers = list(layers)
    if input is None or len(tuple(input)) != 3:
        raise ValueError("Chain: a chain with Conv layers needs its input extent, Chain(..., input=(W, H, C))")
    scale, n = 1.0, 0
    if isinstance(layers[0], Scale):
        scale, n = layers[0].c, 1
    convs = []
    while n < len(layers) and isinstance(layers[n], Conv):
        convs.append(layers[n]); n += 1
    if not convs or n >= len(layers) or not isinstance(layers[n], _Flatten):
        raise ValueError("Chain: a conv chain is [Scale,] Conv..., flatten, Dense... (Scale in the first position only, flatten after the last Conv)")
    if len(convs) > 4:
        raise NotImplementedError("Chain: %d Conv layers, at most 4 are implemented" % len(convs))
    head = layers[n + 1:]
    if not head or any(getattr(l, "conv_kind", None) for l in head) or not all(isinstance(l, Dense) for l in head):
        raise ValueError("Chain: flatten must be followed by Dense layers only (ConvSN, ConvTranspose, pooling and batch norm are not implemented)")
    if any(getattr(l, "n_iterations", 0) for l in head):
        raise NotImplementedError("Chain: DenseSN layers behind a conv trunk are not implemented")
    spec = ConvSpec(input[0], input[1], input[2], scale, convs)
    if head[0].inp != spec.out_features:
        raise ValueError("Chain: flatten yields %d x %d x %d = %d features, the next Dense takes %d" % (spec.extents[-1] + (spec.out_features, head[0].inp)))
    return spec, head


TRUNK_STREAM = 0x40000000      # the trunk's glorot draws use Philox stream `stream + TRUNK_STREAM`: weight n of the trunk and weight n of the head would otherwise be one draw


class ConvTrunk:
    """crux_conv (the layer table and the workspace) + the bare-vector crux_mlp that owns the trunk's parameters, gradient and Adam state"""

    def __init__(self, spec, ctx=None, seed=0, stream=0):
        self.ctx, self.spec = ctx or default_context(), spec
        arr = (L.ConvLayer * len(spec.convs))()
        for a, l in zip(arr, spec.convs):
            a.k1, a.k2, a.cin, a.cout, a.stride1, a.stride2, a.pad1, a.pad2, a.act = l.k + (l.cin, l.cout) + l.stride + l.pad + (L.ACT[l.act],)
            a.dilation1, a.dilation2, a.groups = l.dilation + (l.groups,)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.crux_conv_create(self.ctx.h, spec.W, spec.H, spec.C, spec.scale, len(spec.convs), arr, C.byref(h)))
        self.h = h
        assert int(self.ctx.lib.crux_conv_n_params(self.h)) == spec.n_params and int(self.ctx.lib.crux_conv_out_features(self.h)) == spec.out_features
        self.p = ParamVector(np.zeros(spec.n_params, np.float32), ctx=self.ctx)
        self.ctx.check(self.ctx.lib.crux_conv_init_glorot(self.h, self.p.h, int(seed), (int(stream) + TRUNK_STREAM) & 0xFFFFFFFF))

    def forward(self, s):
        """features [out_features x B] of host observations [W H C x B]"""
        x = np.asfortranarray(s, np.float32)
        if x.ndim == 1:
            x = x.reshape(-1, 1, order="F")
        if x.shape[0] != self.spec.in_features:
            raise ValueError("value: input has %d rows, the trunk takes W H C = %d" % (x.shape[0], self.spec.in_features))
        B = x.shape[1]; y = np.empty((self.spec.out_features, B), np.float32, order="F")
        ctx = self.ctx; d_x, d_y = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes)
        try:
            ctx.h2d(d_x, x)
            ctx.check(ctx.lib.crux_conv_forward(self.h, self.p.h, d_x, B, d_y))
            ctx.d2h(d_y, y)
        finally:
            ctx.free(d_x); ctx.free(d_y)
        return y

    def head_forward(self, head, s):
        """head(trunk(s)) [n_out x B] for host observations: both passes on the device, the head through the dense engine (crux_mlp_forward_cached: the small-MLP kernels
        stop at narrower inputs than a flattened feature map)"""
        x = np.asfortranarray(s, np.float32)
        if x.ndim == 1:
            x = x.reshape(-1, 1, order="F")
        if x.shape[0] != self.spec.in_features:
            raise ValueError("value: input has %d rows, the trunk takes W H C = %d" % (x.shape[0], self.spec.in_features))
        B, nout = x.shape[1], head.network.dims[-1]; y = np.empty((nout, B), np.float32, order="F")
        ctx = self.ctx; d_x, d_f, d_y = ctx.alloc(x.nbytes), ctx.alloc(4 * self.spec.out_features * B), ctx.alloc(y.nbytes)
        try:
            ctx.h2d(d_x, x)
            ctx.check(ctx.lib.crux_conv_forward(self.h, self.p.h, d_x, B, d_f))
            ctx.check(ctx.lib.crux_mlp_forward_cached(head.head_h, d_f, B, d_y))
            ctx.d2h(d_y, y)
        finally:
            for d in (d_x, d_f, d_y):
                ctx.free(d)
        return y

    def explore_tail(self, nout):
        """Dense(n_out, n_out) with the identity matrix and no bias: crux_policy_explore over the head's OUTPUT. The exploration kernels take inputs up to 32 wide, a
        flattened feature map is wider; their draws and head arithmetic depend on the network's output alone, and this layer hands the values on exactly (1 q + 0 ...)."""
        if getattr(self, "_tail", None) is None or self._tail.network.dims[0] != nout:
            from .core import Chain, ContinuousNetwork
            self._tail = ContinuousNetwork(Chain(Dense(nout, nout)), ctx=self.ctx)
            self._tail.set_params(np.concatenate([np.eye(nout, dtype=np.float32).reshape(-1), np.zeros(nout, np.float32)]))
        return self._tail

    def params(self):
        flat, out, off = self.p.get_params(), [], 0
        for shp in self.spec.shapes:
            n = int(np.prod(shp)); out.append(flat[off:off + n].reshape(shp, order="F").copy()); off += n
        return out

    def __del__(self):
        try:
            if getattr(self, "h", None) and self.ctx.h:
                self.ctx.lib.crux_conv_destroy(self.h)
        except Exception:
            pass
