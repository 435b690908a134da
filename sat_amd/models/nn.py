"""NN primitive layer — the single funnel through which every learnable op
is created (parity with reference `utils/nn.py`).

Centralizes:
  * initializer policy — fc kernels uniform ±fc_kernel_initializer_scale
    (nn.py:29-31), conv kernels Xavier (nn.py:15);
  * regularization policy — L2 on fc/conv kernels at the configured scales,
    collected into `reg_loss()` exactly like TF's graph-level
    get_regularization_loss (nn.py:17-43, model.py:328);
  * dropout rates (fc_drop_rate, nn.py:107-114);
  * the freeze-CNN policy — conv/bn parameters are trainable only when
    `config.train_cnn` (nn.py:66), fc parameters only when `is_train`.

Modules created here call into sat_amd.ops, which dispatches to the CDNA4
HIP kernels on GPU and plain PyTorch on CPU.
"""

import math

import torch
import torch.nn as tnn

from .. import ops

# Padded-output chain of the frozen VGG forward: every producer (conv or
# pool) whose consumer is an in-tree padded-input 3x3 conv writes its
# result straight into a 1-px zero-bordered buffer, so no pad1_nhwc pass
# runs between them (profiles/pad_chain_perf_log.md; PAD_CHAIN_8P below
# is the one exception).  False restores the pad1_nhwc routing everywhere
# except conv1_1 -> conv1_2 (which chained before the switch existed); it
# is there for A/B runs and tests.
PAD_CHAIN = True

# Whether the single-pass 8-phase kernel (conv3_x / conv4_x at batch 32)
# also emits padded.  Measured, it should not: its padded epilogue costs
# 24-27 us per layer, the pad1_nhwc pass it would remove 9-17 us
# (profiles/pad_chain_perf_log.md), so those four pad passes stay.  The
# pools, conv1_1, the glds kernel and the split-K combine kernel emit
# padded at (almost) no cost.  True gives the pad-pass-free forward.
PAD_CHAIN_8P = False

# Route of the Cout%256 3x3 convs below the 8-phase kernel's chip-filling
# size (conv5 at batch 32, M = 6272): 'intree' = split-K 8-phase kernel,
# 'miopen' = the library's split-K igemm.  Decided end to end, all helper
# kernels of both routes counted (profiles/pad_chain_perf_log.md).
CONV5_ROUTE = 'intree'
_8P_FULL_M = 12544      # 8-phase single pass fills the chip from here
_8P_SPLIT_M = 6272      # smallest M measured on the split-K route


def _8p_single_pass(Cout, Cin, M):
    """conv_igemm_8p_fwd's own choice (conv8p.hip): True when it runs one
    pass with the bf16 epilogue, False when it splits K and the combine
    kernel writes the output."""
    blocks = -(-Cout // 256) * -(-M // 256)
    return min(8, 224 // blocks, 9 * (Cin // 64) // 2) <= 1


def _unpad(x):
    return x[:, :, 1:-1, 1:-1].contiguous(memory_format=torch.channels_last)


class NN(object):
    """Policy object handed to every layer factory."""

    def __init__(self, config):
        self.config = config
        self.is_train = getattr(config, 'phase', 'train') == 'train'
        self.train_cnn = self.is_train and getattr(config, 'train_cnn', False)
        self.fc_scale = config.fc_kernel_initializer_scale
        self.fc_reg = config.fc_kernel_regularizer_scale \
            if self.is_train else 0.0
        self.conv_reg = config.conv_kernel_regularizer_scale \
            if self.train_cnn else 0.0
        self.fc_drop_rate = config.fc_drop_rate
        self.lstm_drop_rate = config.lstm_drop_rate
        # L1 activity regularizers (reference nn.py:23-27,39-43): applied
        # to the output of every activation-carrying fc/conv layer, gated
        # on is_train (fc) / train_cnn (conv) exactly like the kernels.
        self.fc_act_reg = getattr(
            config, 'fc_activity_regularizer_scale', 0.0) \
            if self.is_train else 0.0
        self.conv_act_reg = getattr(
            config, 'conv_activity_regularizer_scale', 0.0) \
            if self.train_cnn else 0.0
        # (param, scale) pairs for reg_loss; filled as layers are built
        self._regularized = []
        # per-forward activity-loss terms (cleared by reg_loss)
        self._act_losses = []

    def init_fc_(self, t):
        tnn.init.uniform_(t, -self.fc_scale, self.fc_scale)

    def init_conv_(self, t):
        tnn.init.xavier_uniform_(t)

    def register_fc_kernel(self, p):
        if self.fc_reg > 0:
            self._regularized.append((p, self.fc_reg))

    def register_conv_kernel(self, p):
        if self.conv_reg > 0:
            self._regularized.append((p, self.conv_reg))

    def add_activity_loss(self, y, scale):
        """Record scale · Σ|y| for one layer output (TF l1_regularizer
        as activity_regularizer, reference nn.py:23-27,39-43)."""
        if scale > 0 and torch.is_grad_enabled():
            self._act_losses.append(scale * y.float().abs().sum())

    def reg_loss(self):
        """Σ scale · l2_loss(w) (l2_loss = sum(w²)/2, TF semantics) plus
        any activity-regularizer terms recorded this forward.

        On GPU the kernel-L2 term runs as ONE multi-tensor foreach pass
        (a per-param eager loop cost ~55 launches/step)."""
        total = torch.zeros(())
        if self._regularized:
            if self._regularized[0][0].is_cuda:
                params = tuple(p for p, _ in self._regularized)
                scales = tuple(s for _, s in self._regularized)
                total = _RegL2.apply(scales, *params)
            else:
                total = sum(s * 0.5 * (p.float() ** 2).sum()
                            for p, s in self._regularized)
        if self._act_losses:
            act = sum(self._act_losses)
            self._act_losses = []
            total = total.to(act.device) + act
        return total

    def dropout(self, x):
        return ops.dropout(x, self.fc_drop_rate, self.is_train)


class _RegL2(torch.autograd.Function):
    """Multi-tensor Σ scale·0.5·||p||² with closed-form backward
    (d/dp = d·scale·p): ~6 launches forward + one foreach backward
    instead of per-param pow/reduce/mul/add chains."""

    _scale_cache = {}

    @staticmethod
    def forward(ctx, scales, *params):
        ctx.save_for_backward(*params)
        ctx.scales = scales
        norms = torch._foreach_norm(params, 2)
        sv = torch.stack([n.float() for n in norms])
        # cached device constant: creating it per call would be a host
        # copy inside the captured graph
        key = (scales, sv.device)
        sc = _RegL2._scale_cache.get(key)
        if sc is None:
            sc = torch.tensor(scales, dtype=torch.float32,
                              device=sv.device)
            _RegL2._scale_cache[key] = sc
        return (sv * sv * sc * 0.5).sum()

    @staticmethod
    def backward(ctx, d):
        params = ctx.saved_tensors
        gs = torch._foreach_mul(params, list(ctx.scales))
        gs = torch._foreach_mul(gs, d)
        return (None, *gs)


class Dense(tnn.Module):
    """tf.layers.dense analog (reference nn.py:85-105); kernel stored
    [out, in] (torch layout) for transpose-free MFMA consumption."""

    def __init__(self, nn_policy, in_dim, units, activation='tanh',
                 use_bias=True):
        super().__init__()
        self.activation = activation
        self._nn = nn_policy
        self.weight = tnn.Parameter(torch.empty(units, in_dim))
        nn_policy.init_fc_(self.weight)
        nn_policy.register_fc_kernel(self.weight)
        if use_bias:
            self.bias = tnn.Parameter(torch.zeros(units))
        else:
            self.register_parameter('bias', None)
        self._wc = None  # per-forward cast cache (set by precast())
        self._bc = None

    def precast(self, dtype):
        """Cast weights once per model forward; the cast stays in the
        autograd graph, so T uses of the layer accumulate into one fp32
        parameter grad (like TF's reuse_variables, model.py:312)."""
        self._wc = self.weight.to(dtype)
        self._bc = self.bias.to(dtype) if self.bias is not None else None

    def clear_cast(self):
        self._wc = None
        self._bc = None

    def forward(self, x):
        if self._wc is not None and self._wc.dtype == x.dtype:
            y = ops.dense(x, self._wc, self._bc, self.activation)
        else:
            w = self.weight.to(x.dtype)
            b = self.bias.to(x.dtype) if self.bias is not None else None
            y = ops.dense(x, w, b, self.activation)
        # activity regularizer only on activation-carrying layers
        # (reference nn.py:92-95)
        if self.activation is not None and self._nn.fc_act_reg > 0:
            self._nn.add_activity_loss(y, self._nn.fc_act_reg)
        return y


class _WatchedParameter(tnn.Parameter):
    """A parameter that counts the accesses to its `.data`.

    `p.data` is an alias with a version counter of its own, so a write
    through it (`p.data.copy_(...)`) leaves `p._version` where it was and
    a cache keyed on `_version` alone would go stale.  Conv2d keys its
    cast cache on this count as well and treats every access as a possible
    write.  Nothing on the training path reads `.data` of a frozen
    parameter, so the cache is not disturbed there.

    Limits: an alias taken earlier (`d = p.data`) and written to after
    the cast was cached is not seen, nor is a raw-pointer write by a
    kernel; and a pickled parameter comes back as a plain Parameter, whose
    cache then follows `_version` alone.  Code that writes a frozen conv
    parameter in such a way sets `conv._cast_cache = None`."""

    _data_reads = 0

    @property
    def data(self):
        self._data_reads += 1
        return torch.Tensor.data.__get__(self)

    @data.setter
    def data(self, value):
        self._data_reads += 1
        torch.Tensor.data.__set__(self, value)


class Conv2d(tnn.Module):
    """conv2d + bias + optional ReLU (reference nn.py:45-70 defaults:
    3x3, stride 1, SAME padding, ReLU)."""

    def __init__(self, nn_policy, in_ch, out_ch, kernel_size=3, stride=1,
                 activation='relu', use_bias=True):
        super().__init__()
        self.stride = stride
        self.kernel_size = kernel_size
        self.activation = activation
        self._nn = nn_policy
        self._glds_conv = getattr(nn_policy.config, 'use_glds_conv',
                                  True)
        self._cast_cache_on = getattr(nn_policy.config,
                                      'cache_frozen_conv_cast', True)
        self.weight = _WatchedParameter(
            torch.empty(out_ch, in_ch, kernel_size, kernel_size))
        nn_policy.init_conv_(self.weight)
        nn_policy.register_conv_kernel(self.weight)
        if use_bias:
            self.bias = _WatchedParameter(torch.zeros(out_ch))
        else:
            self.register_parameter('bias', None)

    def _igemm_route(self, M, padded_in=False):
        """Frozen-GPU implicit-GEMM kernel for this 3x3/s1 layer at M
        output pixels: '8p', 'glds', 'g64' (all three read a 1-px padded
        input), 'ig64' (unpadded input) or None (library conv).

        Per-shape winners (profiles/r01_conv_shapes.txt, r02 8-phase
        kernel, profiles/pad_chain_perf_log.md for conv5):
          * Cout%256==0 with enough output pixels to fill the chip at a
            256^2 tile: the 8-phase deep-pipelined igemm (conv8p.hip) —
            the Cin>=256 layers MIOpen used to keep; below that, down to
            conv5 at batch 32, its split-K form when CONV5_ROUTE says so;
          * Cin<=128 & Cout>=128: the XOR-swizzled glds variant
            (120 vs 169 us on conv2_1);
          * Cout<128 (conv1_2): glds64, 525 TF vs the register igemm's
            350 (profiles/r02_conv_shapes.txt);
          * Cin=64 without `use_glds_conv`: register-staged MFMA conv.
        `use_glds_conv` gates all LDS-DMA-staged variants."""
        Cout, Cin = self.weight.shape[0], self.weight.shape[1]
        if (self.kernel_size != 3 or self.stride != 1
                or Cout % 8 != 0 or Cin % 8 != 0):
            return None
        if self._glds_conv and Cin % 64 == 0:
            min_m = _8P_SPLIT_M if CONV5_ROUTE == 'intree' else _8P_FULL_M
            if Cout % 256 == 0 and M >= min_m:
                return '8p'
            if Cout >= 128 and Cin <= 128:
                return 'glds'
            if Cout < 128:
                return 'g64'
        if Cin == 64 and not padded_in:
            return 'ig64'
        return None

    def _accepts_padded(self, M):
        """Will forward() consume a 1-px padded input directly (frozen
        GPU bf16 forward assumed, as in the producer that asks)?"""
        return (getattr(self, '_accept_padded', False)
                and self._igemm_route(M, True) in ('8p', 'glds', 'g64'))

    def _emits_padded(self, M):
        """Emit a padded output for the consumer wired by the encoder?
        conv1_1 -> conv1_2 chained before PAD_CHAIN existed and stays on
        with the switch off."""
        if not (getattr(self, '_emit_padded', False) and self._glds_conv):
            return False
        if not (PAD_CHAIN or self.weight.shape[1] == 3):
            return False
        ok = getattr(self, '_pad_consumer_ok', None)
        return ok is None or ok(M)

    def _cast_operands(self, dtype):
        """Weight and bias in the compute dtype.  A frozen layer (no grad
        mode, parameters that do not require grad) casts once and keeps
        the result until a parameter is written to (`_version`, as for
        `_w_ohwi`, and the `.data` accesses of _WatchedParameter), moved,
        or the dtype changes; every other caller gets a fresh cast that
        stays in the autograd graph."""
        w, b = self.weight, self.bias
        frozen = (self._cast_cache_on and not torch.is_grad_enabled()
                  and not w.requires_grad
                  and (b is None or not b.requires_grad))
        if not frozen:
            return w.to(dtype), (b.to(dtype) if b is not None else None)
        key = (w._version, getattr(w, '_data_reads', 0),
               b._version if b is not None else -1,
               getattr(b, '_data_reads', 0), dtype,
               w.device, w.data_ptr(), w.stride())
        cache = getattr(self, '_cast_cache', None)
        if cache is None or cache[0] != key:
            cache = (key, w.to(dtype), b.to(dtype) if b is not None else None)
            self._cast_cache = cache
        return cache[1], cache[2]

    def forward(self, x):
        w, b = self._cast_operands(x.dtype)
        k, st = self.kernel_size, self.stride
        # chained-pad handshake: a producing conv or pool may hand over a
        # 1-px zero-bordered output (tagged `_sat_pad`); a 3x3/s1 consumer
        # marked _accept_padded uses it directly, anyone else unpads
        pad_hw = getattr(x, '_sat_pad', None)
        if pad_hw is not None and not (
                getattr(self, '_accept_padded', False)
                and k == 3 and st == 1
                and not torch.is_grad_enabled()):
            x = _unpad(x)
            pad_hw = None
        # --train_cnn: hand-written forward/dgrad/wgrad autograd triple
        # (reference model.py:505-511 backward surface on in-tree kernels)
        if (torch.is_grad_enabled()
                and (x.requires_grad or w.requires_grad)
                and self._glds_conv and k == 3 and st == 1
                and self.activation in ('relu', None)):
            from ..ops.convgrad import Conv3x3Train, conv3x3_train_ok
            if conv3x3_train_ok(x, w):
                y = Conv3x3Train.apply(x, w, b,
                                       self.activation == 'relu')
                if self.activation is not None \
                        and self._nn.conv_act_reg > 0:
                    self._nn.add_activity_loss(y, self._nn.conv_act_reg)
                return y
        if (x.is_cuda and x.dtype == torch.bfloat16
                and not torch.is_grad_enabled()
                and k == 3 and st == 1 and w.shape[1] == 3
                and w.shape[0] % 8 == 0 and w.shape[0] <= 128
                and x.is_contiguous(memory_format=torch.channels_last)):
            # 3-channel first layer: MIOpen NHWC bf16 falls back to a
            # 2.4 ms CK kernel here; the direct kernel is memory-bound
            from ..ops import hip
            if hip.available():
                from sat_amd import _C
                emit = self._emits_padded(
                    x.shape[0] * x.shape[2] * x.shape[3])
                y = _C.conv3_fwd(
                    x, w.contiguous(),
                    b if b is not None
                    else torch.empty(0, dtype=x.dtype, device=x.device),
                    self.activation == 'relu', emit)
                if emit:
                    y._sat_pad = (x.shape[2], x.shape[3])
                return y
        # frozen GPU implicit-GEMM paths, routed per shape by
        # _igemm_route()
        if (x.is_cuda and x.dtype == torch.bfloat16
                and not torch.is_grad_enabled()
                and k == 3 and st == 1
                and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0
                and x.is_contiguous(memory_format=torch.channels_last)):
            from ..ops import hip
            if hip.available():
                from sat_amd import _C
                H = pad_hw[0] if pad_hw else x.shape[2]
                W = pad_hw[1] if pad_hw else x.shape[3]
                M = x.shape[0] * H * W
                relu = self.activation == 'relu'
                route = self._igemm_route(M, pad_hw is not None)
                if route is not None:
                    if getattr(self, '_w_ohwi', None) is None or \
                            self._w_ohwi_ver != self.weight._version:
                        self._w_ohwi_ver = self.weight._version
                        self._w_ohwi = w.permute(0, 2, 3, 1).contiguous() \
                            .reshape(w.shape[0], -1)
                    eb = (b if b is not None else
                          torch.empty(0, dtype=x.dtype, device=x.device))
                    if route == 'ig64':
                        return _C.conv_igemm_fwd(x, self._w_ohwi, eb,
                                                 relu)
                    xp = x if pad_hw is not None else _C.pad1_nhwc(x)
                    # the epilogue writes the next conv's zero border
                    # itself when the encoder wired one that takes it
                    emit = self._emits_padded(M) and (
                        route != '8p' or PAD_CHAIN_8P
                        or not _8p_single_pass(w.shape[0], w.shape[1], M))
                    fwd = {'8p': _C.conv_igemm_8p_fwd,
                           'glds': _C.conv_igemm_glds_fwd,
                           'g64': _C.conv_igemm_glds64_fwd}[route]
                    y = fwd(xp, self._w_ohwi, eb, H, W, relu, emit)
                    if emit:
                        y._sat_pad = (H, W)
                    return y
        # 1x1/s1 conv IS a GEMM over the NHWC row view: route through
        # the in-tree tiled MFMA GEMM instead of MIOpen (ResNet50's
        # bottleneck convs; bias handled by the GEMM epilogue)
        if (x.is_cuda and x.dtype == torch.bfloat16
                and not torch.is_grad_enabled()
                and k == 1 and st == 1 and pad_hw is None
                and self._glds_conv
                and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0
                and x.is_contiguous(memory_format=torch.channels_last)):
            from ..ops import hip
            if hip.available():
                from sat_amd import _C
                B_, Cin, H, W = x.shape
                Cout = w.shape[0]
                rows = x.permute(0, 2, 3, 1).reshape(B_ * H * W, Cin)
                if getattr(self, '_w_1x1', None) is None or \
                        self._w_1x1_ver != self.weight._version:
                    self._w_1x1_ver = self.weight._version
                    self._w_1x1 = w.reshape(Cout, Cin).contiguous()
                eb = (b if b is not None else
                      torch.empty(0, dtype=x.dtype, device=x.device))
                act = 2 if self.activation == 'relu' else 0
                y = _C.dense_fwd(rows, self._w_1x1, eb, act)
                return y.reshape(B_, H, W, Cout).permute(0, 3, 1, 2)
        if pad_hw is not None:
            # padded input fell through to a library path: unpad first
            x = x[:, :, 1:-1, 1:-1] \
                .contiguous(memory_format=torch.channels_last)
        # frozen GPU path: fused NHWC bias+ReLU kernel after the MIOpen
        # conv instead of two separate eager elementwise passes
        fuse_epi = (x.is_cuda and x.dtype == torch.bfloat16
                    and not torch.is_grad_enabled() and b is not None
                    and self.weight.shape[0] % 8 == 0)
        conv_bias = None if fuse_epi else b
        ph = _same_pad(x.shape[2], k, st)
        pw = _same_pad(x.shape[3], k, st)
        if ph % 2 == 0 and pw % 2 == 0:
            # symmetric SAME: no pad-copy kernel, pad inside the conv
            y = torch.nn.functional.conv2d(x, w, conv_bias, stride=st,
                                           padding=(ph // 2, pw // 2))
        else:
            x = torch.nn.functional.pad(
                x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
            y = torch.nn.functional.conv2d(x, w, conv_bias, stride=st)
        if fuse_epi and y.is_contiguous(
                memory_format=torch.channels_last):
            from ..ops import hip
            if hip.available():
                from sat_amd import _C
                _C.bias_act_nhwc(y, b, self.activation == 'relu')
                return y
            y = y + b.reshape(1, -1, 1, 1)
        elif fuse_epi:
            y = y + b.reshape(1, -1, 1, 1)
        if self.activation == 'relu':
            y = torch.relu(y)
        # conv activity regularizer (reference nn.py:54-57): only on
        # activation-carrying layers, only when the CNN trains — which is
        # exactly when this autograd path (not the inference kernels) runs
        if self.activation is not None and self._nn.conv_act_reg > 0:
            self._nn.add_activity_loss(y, self._nn.conv_act_reg)
        return y


def _same_pad(size, k, s):
    out = math.ceil(size / s)
    return max((out - 1) * s + k - size, 0)


def _pad_same(x, k, s):
    """TF 'SAME' padding (asymmetric: extra on bottom/right)."""
    ph = _same_pad(x.shape[2], k, s)
    pw = _same_pad(x.shape[3], k, s)
    if ph == 0 and pw == 0:
        return x
    return torch.nn.functional.pad(
        x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))


class MaxPool2d(tnn.Module):
    """max_pool2d 2x2 s2 SAME (reference nn.py:72-83)."""

    def __init__(self, kernel_size=2, stride=2):
        super().__init__()
        self.kernel_size = kernel_size
        self.stride = stride

    def forward(self, x):
        if getattr(x, '_sat_pad', None) is not None:
            x = _unpad(x)           # pools read unpadded input only
        if (x.is_cuda and x.dtype == torch.bfloat16
                and not torch.is_grad_enabled()
                and self.kernel_size == 2 and self.stride == 2
                and x.shape[1] % 8 == 0
                and x.is_contiguous(memory_format=torch.channels_last)):
            from ..ops import hip
            if hip.available():
                from sat_amd import _C
                # padded-output chain (PAD_CHAIN): write the next conv's
                # zero border here when the encoder wired one that takes it
                Ho, Wo = (x.shape[2] + 1) // 2, (x.shape[3] + 1) // 2
                ok = getattr(self, '_pad_consumer_ok', None)
                emit = bool(PAD_CHAIN
                            and getattr(self, '_emit_padded', False)
                            and ok is not None
                            and ok(x.shape[0] * Ho * Wo))
                y = _C.maxpool2x2_nhwc(x, emit)
                if emit:
                    y._sat_pad = (Ho, Wo)
                return y
        x = _pad_same(x, self.kernel_size, self.stride)
        return torch.nn.functional.max_pool2d(
            x, self.kernel_size, self.stride)


class BatchNorm(tnn.Module):
    """batch_norm gated on train_cnn (reference nn.py:116-125).

    Frozen GPU path: inference BN is a fixed per-channel scale/shift
    (scale = gamma/sqrt(var+eps), shift = beta - mean*scale), applied by
    ONE NHWC kernel with optional fused ReLU — instead of the eager
    fp32-cast + BN + bf16-cast chain (3 kernels x 53 BNs on ResNet50)."""

    def __init__(self, nn_policy, num_features):
        super().__init__()
        self.train_cnn = nn_policy.train_cnn
        self.bn = tnn.BatchNorm2d(num_features, eps=1e-3, momentum=0.01)
        self._ss = None  # cached (scale, shift) bf16 (frozen only)

    def forward(self, x, relu=False):
        if self.train_cnn:
            y = self.bn(x.float()).to(x.dtype)
            return torch.relu(y) if relu else y
        if (x.is_cuda and x.dtype == torch.bfloat16
                and not torch.is_grad_enabled()
                and x.shape[1] % 8 == 0
                and x.is_contiguous(memory_format=torch.channels_last)):
            from ..ops import hip
            if hip.available():
                from sat_amd import _C
                # all four stat/affine tensors key the cache: a partial
                # load_cnn/checkpoint match may in-place update only
                # running_mean or bias, which must invalidate too
                ver = (self.bn.running_var._version,
                       self.bn.running_mean._version,
                       self.bn.weight._version,
                       self.bn.bias._version)
                if (self._ss is None or self._ss[0].device != x.device
                        or getattr(self, '_ss_ver', None) != ver):
                    self._ss_ver = ver
                    bn = self.bn
                    scale = (bn.weight /
                             torch.sqrt(bn.running_var + bn.eps))
                    shift = bn.bias - bn.running_mean * scale
                    self._ss = (scale.to(x.device, torch.bfloat16)
                                .contiguous(),
                                shift.to(x.device, torch.bfloat16)
                                .contiguous())
                _C.scale_bias_act_nhwc(x, self._ss[0], self._ss[1], relu)
                return x
        training = self.bn.training
        self.bn.eval()
        y = self.bn(x.float()).to(x.dtype)
        if training:
            self.bn.train()
        return torch.relu(y) if relu else y
