"""
The optimizer over a ``HipNetwork``'s flat parameter as the library's own kernel (csrc/mzx_optim.h, ``mzx_optim_step``).

``mzx.optim.Adam`` and ``mzx.optim.SGD`` subclass ``torch.optim.Adam`` / ``torch.optim.SGD`` and override ``step()``
alone: ``param_groups``, ``state``, ``state_dict()``, ``load_state_dict()`` and ``zero_grad()`` stay torch's, with the state
keys and dtypes torch creates (``step``, ``exp_avg``, ``exp_avg_sq``, ``momentum_buffer``), so ``mzx.trainer.update_lr``,
``optimizer_state`` / ``load_optimizer_state`` and a checkpoint in the reference's format work unchanged.

    optimizer = mzx.optim.Adam(model.parameters(), lr=config.lr_init, weight_decay=config.weight_decay)
    optimizer = mzx.optim.SGD(model, lr=config.lr_init, momentum=config.momentum, weight_decay=config.weight_decay)
    optimizer = mzx.optim.from_config(model, config)          # trainer.py:36-53

A step is ONE launch that visits only the live spans of the flat buffer: ``running_mean`` / ``running_var`` (buffers in
the reference, never an optimizer's business) and, behind a downsample stem, the ``representation_network.module.conv`` /
``.bn`` tensors the stem bypasses (``.grad`` is None there in the reference) are neither read nor written -- the
parameter, the gradient and the state alike; the state over them stays exactly zero.  The arithmetic is the definition in
include/mzx.h (binary32, nothing fused): torch's float32 result within its own rounding error, not bit for bit.

The flat parameter leads back to its network (``HipNetwork`` ties itself to the ``Parameter`` it hands out); any other
parameter raises ``ValueError``.  What the kernel does not implement raises ``NotImplementedError`` by name at
construction: more than one param group, ``amsgrad``, ``maximize``, ``nesterov``, ``dampening != 0``, and the
``capturable`` / ``differentiable`` / ``fused`` / ``foreach`` flags set to anything but their defaults.
"""
import ctypes

import numpy
import torch

from . import _lib, models

_FLAG_DEFAULTS = dict(foreach=None, maximize=False, capturable=False, differentiable=False, fused=None)
_BYPASSED = ("representation_network.module.conv.", "representation_network.module.bn.")      # with config.downsample


def live_spans(net):
    """The (offset, count) spans of ``net``'s flat buffer an optimizer updates, neighbours joined: every tensor of
    ``mzx_net_tensor_info`` but ``running_mean`` / ``running_var`` and, with a downsample stem, those under ``_BYPASSED``."""
    spans = []
    for key, off, numel, _ in net._tensors:
        if key.endswith((".running_mean", ".running_var")) or (net._cfg.downsample and key.startswith(_BYPASSED)):
            continue
        if spans and spans[-1][0] + spans[-1][1] == off:
            spans[-1][1] += numel
        else:
            spans.append([off, numel])
    return [tuple(s) for s in spans]


class SpanTable:
    """The host span array and the device chunk table of a network (``mzx_optim_chunks``), built once."""

    def __init__(self, net):
        be = net.backend
        self.spans = live_spans(net)
        self.h_spans = numpy.ascontiguousarray(numpy.asarray(self.spans, dtype=numpy.int64).reshape(-1, 2))
        n = int(net.num_params)
        count = int(be.lib.mzx_optim_chunks(self.h_spans.ctypes.data, len(self.h_spans), n, None, 0))
        if count < 0:
            be.lib.check(count)
        chunks = numpy.zeros((max(count, 1), 2), dtype=numpy.int64)
        be.lib.mzx_optim_chunks(self.h_spans.ctypes.data, len(self.h_spans), n, chunks.ctypes.data, count)
        self.d_chunks = torch.from_numpy(chunks).to(be.device)
        self.num_chunks = count

    def fill(self, io):
        io.h_spans, io.num_spans = self.h_spans.ctypes.data, len(self.h_spans)
        io.d_chunks, io.num_chunks = self.d_chunks.data_ptr(), self.num_chunks


def span_table(net):
    table = getattr(net, "_optim_table", None)
    if table is None:
        table = net._optim_table = SpanTable(net)
    return table


def network_of(param):
    """The ``HipNetwork`` whose flat parameter ``param`` is, or ValueError."""
    ref = getattr(param, "_mzx_network", None)
    net = ref() if ref is not None else None
    if net is None or next(net.parameters()) is not param:
        raise ValueError("mzx.optim: the parameter is not the flat parameter of a HipNetwork (pass model.parameters() of a "
                         "mzx.models.MuZeroNetwork, or the network itself)")
    return net


def _flat_parameter(who, params):
    """``params`` as the constructors take them -> (network, [its flat parameter])."""
    if isinstance(params, models.HipNetwork):
        params = params.parameters()
    params = list(params)
    if params and isinstance(params[0], dict):
        if len(params) != 1:
            raise NotImplementedError(f"mzx.optim.{who}: more than one param group ({len(params)} given) is not implemented")
        extra = sorted(k for k in params[0] if k != "params")
        if extra:
            raise NotImplementedError(f"mzx.optim.{who}: per-group options ({', '.join(extra)}) are not implemented")
        params = params[0]["params"]
        params = [params] if torch.is_tensor(params) else list(params)
    if len(params) != 1:
        raise ValueError(f"mzx.optim.{who}: expected the one flat parameter of a HipNetwork, got {len(params)} parameters")
    return network_of(params[0]), params


def _refuse(who, options, defaults):
    for key, value in options.items():
        if key not in defaults:
            raise TypeError(f"mzx.optim.{who}: unexpected keyword argument '{key}'")
        if value is not defaults[key] and value != defaults[key]:
            raise NotImplementedError(f"mzx.optim.{who}: {key}={value!r} is not implemented by the native kernel")


def _scalar(who, name, value):
    if torch.is_tensor(value):
        raise NotImplementedError(f"mzx.optim.{who}: a tensor {name} is not implemented (capturable / fused territory); pass a float")
    return float(value)


class _Native:
    """What the two classes share: the one group and parameter, its network, the io struct of a step."""

    def _io(self, kind, who, refusals):
        if len(self.param_groups) != 1 or len(self.param_groups[0]["params"]) != 1:
            raise NotImplementedError(f"mzx.optim.{who}: more than one param group / parameter is not implemented")
        group = self.param_groups[0]
        _refuse(who, {k: group[k] for k in refusals if k in group}, refusals)      # (a loaded state_dict may carry them)
        param = group["params"][0]
        net = network_of(param)
        if param.grad is None:
            return group, param, net, None
        grad = param.grad
        if grad.dtype != torch.float32 or grad.shape != param.shape or not grad.is_contiguous() or grad.is_sparse:
            raise ValueError(f"mzx.optim.{who}: .grad must be a dense contiguous float32 tensor of the parameter's shape")
        io = _lib.OptimIO()
        io.kind, io.n = kind, param.numel()
        io.d_param, io.d_grad = param.data_ptr(), grad.data_ptr()
        io.weight_decay = _scalar(who, "weight_decay", group["weight_decay"])
        span_table(net).fill(io)
        return group, param, net, io

    @staticmethod
    def _state_array(who, key, value, param):
        if (not torch.is_tensor(value) or value.dtype != torch.float32 or value.shape != param.shape or value.device != param.device
                or not value.is_contiguous()):
            raise ValueError(f"mzx.optim.{who}: state['{key}'] must be a contiguous float32 tensor like the parameter")
        return value

    @staticmethod
    def _launch(net, io):
        be = net.backend
        be.lib.check(be.lib.mzx_optim_step(ctypes.byref(io), be.stream()))


class Adam(_Native, torch.optim.Adam):
    """``torch.optim.Adam`` whose ``step()`` is one ``mzx_optim_step`` launch over the live spans of the flat buffer."""

    _REFUSED = dict(_FLAG_DEFAULTS, amsgrad=False, decoupled_weight_decay=False)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **flags):
        _refuse("Adam", dict(flags, amsgrad=amsgrad), self._REFUSED)
        _, params = _flat_parameter("Adam", params)
        super().__init__(params, lr=_scalar("Adam", "lr", lr), betas=tuple(_scalar("Adam", "beta", b) for b in betas), eps=eps,
                         weight_decay=weight_decay)

    def adam_scalars(self, t, lr=None):
        """The binary64 scalars of step ``t`` as torch computes them (``_single_tensor_adam``) -> (step_size,
        bias_correction2_sqrt)."""
        group = self.param_groups[0]
        beta1, beta2 = group["betas"]
        lr = _scalar("Adam", "lr", group["lr"]) if lr is None else lr
        bias_correction1 = 1 - beta1 ** t
        bias_correction2 = 1 - beta2 ** t
        return lr / bias_correction1, bias_correction2 ** 0.5

    def native_state(self, create=True):
        """(step tensor, exp_avg, exp_avg_sq) of the flat parameter, created as torch creates them (zeros; ``step`` a 0-d
        float32 tensor on the host)."""
        param = self.param_groups[0]["params"][0]
        state = self.state[param]
        if len(state) == 0 and create:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
        if state["step"].device.type != "cpu":
            raise NotImplementedError("mzx.optim.Adam: a step counter on the device (capturable / fused) is not implemented")
        return (state["step"], self._state_array("Adam", "exp_avg", state["exp_avg"], param),
                self._state_array("Adam", "exp_avg_sq", state["exp_avg_sq"], param))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group, param, net, io = self._io(_lib.OPTIM_ADAM, "Adam", self._REFUSED)
        if io is None:
            return loss
        step, exp_avg, exp_avg_sq = self.native_state()
        step += 1
        t = int(step.item())
        beta1, beta2 = group["betas"]
        io.t, io.d_state1, io.d_state2 = t, exp_avg.data_ptr(), exp_avg_sq.data_ptr()
        io.one_minus_beta1, io.beta2, io.one_minus_beta2, io.eps = 1 - beta1, beta2, 1 - beta2, group["eps"]
        io.step_size, io.bias_correction2_sqrt = self.adam_scalars(t)
        self._launch(net, io)
        return loss


class SGD(_Native, torch.optim.SGD):
    """``torch.optim.SGD`` whose ``step()`` is one ``mzx_optim_step`` launch over the live spans of the flat buffer."""

    _REFUSED = dict(_FLAG_DEFAULTS, nesterov=False, dampening=0)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **flags):
        _refuse("SGD", dict(flags, nesterov=nesterov, dampening=dampening), self._REFUSED)
        _, params = _flat_parameter("SGD", params)
        super().__init__(params, lr=_scalar("SGD", "lr", lr), momentum=momentum, weight_decay=weight_decay)

    def native_state(self):
        """(momentum_buffer, whether this call created it): zeros like the parameter, as no step has written it yet."""
        param = self.param_groups[0]["params"][0]
        state = self.state[param]
        first = state.get("momentum_buffer") is None
        if first:
            state["momentum_buffer"] = torch.zeros_like(param, memory_format=torch.preserve_format)
        return self._state_array("SGD", "momentum_buffer", state["momentum_buffer"], param), first

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group, param, net, io = self._io(_lib.OPTIM_SGD, "SGD", self._REFUSED)
        if io is None:
            return loss
        io.t, io.lr, io.momentum = 1, _scalar("SGD", "lr", group["lr"]), float(group["momentum"])
        if group["momentum"] != 0:
            buf, first = self.native_state()
            io.d_state1, io.first_step = buf.data_ptr(), int(first)
        self._launch(net, io)
        return loss


NATIVE = (Adam, SGD)


def from_config(model, config):
    """trainer.py:36-53: the optimizer ``config.optimizer`` names over ``model``'s flat parameter, natively."""
    if config.optimizer == "SGD":
        return SGD(model.parameters(), lr=config.lr_init, momentum=config.momentum, weight_decay=config.weight_decay)
    if config.optimizer == "Adam":
        return Adam(model.parameters(), lr=config.lr_init, weight_decay=config.weight_decay)
    raise NotImplementedError(f"{config.optimizer} is not implemented. You can change the optimizer manually in trainer.py.")
