"""
The loss head of the trainer on the device (csrc/mzx_trainer.h, ``mzx_trainer_loss``).

``mzx.replay.trainer_tensors`` hands the trainer a batch that never left HBM (trainer.py:140-153); this module is the next
link of ``Trainer.update_weights``: everything between the network's logits and ``loss.backward()`` (trainer.py:161-258)
-- two ``scalar_to_support`` calls, three ``LogSoftmax * target -> sum`` chains and three ``register_hook`` closures per
unroll step, the PER weights, the batch mean, and a blocking ``support_to_scalar(...).cpu()`` per unroll step for the
priorities -- as one library call that returns the loss, the three logged means, the PER priorities and the gradient of
the loss with respect to every head logit.  ``muzero_loss`` wraps it in a ``torch.autograd.Function``: the model, the
optimizer and ``loss.backward()`` stay the caller's, the network's forward and backward stay torch's.

    loss, value_loss, reward_loss, policy_loss, priorities = mzx.trainer.muzero_loss(
        values, rewards, policy_logits,                     # lists of the K + 1 per-step head outputs, or stacked
        target_value, target_reward, target_policy, weight_batch, gradient_scale_batch, config)
    loss.backward()

``update_weights(model, optimizer, batch, config)`` is ``Trainer.update_weights`` with ``self`` unbound;
``train_step(model, optimizer, replay_buffer, config)`` is the whole step on the device: batch drawn by the replay
store's sampler, priorities scattered back into it, no download.  Like the rest
of the package there is no CPU execution path: without the library or a GPU the calls raise as ``default_backend()`` does.

With a ``mzx.models.HipNetwork`` of a fully connected configuration as ``model`` the network is the library's too: the
prediction loop, the loss head and ``loss.backward()`` are ONE ``mzx_train_fc_step`` call (csrc/mzx_train_fc.h, five
launches) that writes ``.grad`` of the network's flat parameter; ``optimizer.step()`` then updates the very buffer self-play
searches on and RCCL broadcasts.  A residual ``HipNetwork`` (no downsample stem) takes the same route through
``mzx_train_resnet_step`` (csrc/mzx_train_resnet.h): BatchNorm in training mode, the convolutions as implicit GEMMs on the
FP32 matrix pipes; after ``optimizer.step()`` the new running statistics are committed into the flat buffer.
A configuration with a downsample stem (``downsample = "resnet"`` / ``"CNN"``: breakout, atari) is refused by name unless
``config.train_downsample = True`` (read by ``models.MuZeroNetwork(config)``) or ``HipNetwork.train_stem = True`` switched
the stem's training on for that handle (``mzx_net_set_train_stem``); then the strided and biased convolutions, the stem's
BatchNorm blocks and its three kinds of pool are trained as well, and the ``representation_network.module.conv`` / ``.bn``
the stem bypasses keep zero gradients, their statistics and their ``num_batches_tracked``.
``update_lr`` is the reference's schedule; ``optimizer_state`` / ``load_optimizer_state``
convert between the flat optimizer state and the reference's per-parameter ``state_dict`` (checkpoints round-trip).
"""
import collections
import copy
import ctypes
import time

import numpy
import torch

from . import _lib, models, optim, replay
from .replay import _remote


def _backend(backend):
    return backend if backend is not None else _lib.default_backend()


def _f32(be, t):
    """``.float()`` on the backend's device, contiguous, cut from the graph."""
    return t.detach().to(be.device, torch.float32).contiguous()


def scalar_to_support(x, support_size, backend=None):
    """
    models.scalar_to_support (models.py:669-689) on the device: ``x`` [batch, steps] -> [batch, steps, 2 * support_size
    + 1] float32, the reference's float32 rows bit for bit (``mzx_scalar_to_support``).
    """
    be = _backend(backend)
    support_size = int(support_size)
    xs = _f32(be, x)
    out = be.empty(tuple(xs.shape) + (2 * support_size + 1,), torch.float32)
    be.lib.check(be.lib.mzx_scalar_to_support(be.ptr(xs), xs.numel(), support_size, be.ptr(out), be.stream()))
    return out


def _run(be, value, reward, policy, target_value, target_reward, target_policy, weight, scale, support_size,
         value_loss_weight, per_alpha, want_grads):
    """One ``mzx_trainer_loss`` call on the backend's current stream.  Returns (packed [4 + B * steps]: the four losses,
    then the priorities; the three gradient buffers or None)."""
    lib = be.lib
    steps, batch, width = value.shape
    actions = policy.shape[2]
    if width != 2 * support_size + 1 or reward.shape != value.shape or policy.shape[:2] != (steps, batch):
        raise ValueError(f"logits: expected value / reward [{steps}, {batch}, {2 * support_size + 1}] and policy "
                         f"[{steps}, {batch}, A], got {tuple(value.shape)}, {tuple(reward.shape)}, {tuple(policy.shape)}")
    if (target_value.shape != (batch, steps) or target_reward.shape != (batch, steps) or scale.shape != (batch, steps)
            or target_policy.shape != (batch, steps, actions) or (weight is not None and weight.shape != (batch,))):
        raise ValueError("targets: expected value / reward / gradient scale [batch, steps], policy [batch, steps, A], weight [batch]")
    packed = be.empty((4 + batch * steps,), torch.float32)
    scratch_bytes = int(lib.mzx_trainer_loss_scratch_bytes(batch, steps))
    scratch = be.empty((scratch_bytes // 4,), torch.float32)
    grads = tuple(torch.empty_like(t) for t in (value, reward, policy)) if want_grads else None
    io = _lib.TrainerLossIO()
    io.d_value_logits, io.d_reward_logits, io.d_policy_logits = value.data_ptr(), reward.data_ptr(), policy.data_ptr()
    io.d_target_value, io.d_target_reward, io.d_target_policy = (target_value.data_ptr(), target_reward.data_ptr(),
                                                                 target_policy.data_ptr())
    io.d_gradient_scale = scale.data_ptr()
    io.d_weight = None if weight is None else weight.data_ptr()
    io.batch, io.steps, io.support_size, io.num_actions = batch, steps, support_size, actions
    io.value_loss_weight, io.per_alpha = float(value_loss_weight), float(per_alpha)
    io.d_losses, io.d_priorities = packed.data_ptr(), packed[4:].data_ptr()
    if grads is not None:
        io.d_grad_value, io.d_grad_reward, io.d_grad_policy = (g.data_ptr() for g in grads)
    io.d_scratch, io.scratch_bytes = scratch.data_ptr(), scratch_bytes
    lib.check(lib.mzx_trainer_loss(ctypes.byref(io), be.stream()))
    return packed, grads


class _MuZeroLoss(torch.autograd.Function):
    """loss = f(value logits, reward logits, policy logits); the library call of ``forward`` already wrote df / dlogits."""

    @staticmethod
    def forward(ctx, value, reward, policy, be, targets, scalars):
        shapes = (value.shape, reward.shape)
        v, r, p = _f32(be, value), _f32(be, reward), _f32(be, policy)
        if v.dim() == 4 and v.shape[-1] == 1:          # the reference squeezes a trailing singleton (trainer.py:187-188)
            v = v.squeeze(-1)
        if r.dim() == 4 and r.shape[-1] == 1:
            r = r.squeeze(-1)
        if v.dim() != 3 or r.dim() != 3 or p.dim() != 3:
            raise ValueError("logits must be [steps, batch, width] (or lists of per-step [batch, width] tensors)")
        want = any(ctx.needs_input_grad[:3])
        packed, grads = _run(be, v, r, p, *targets, *scalars, want)
        ctx.grads, ctx.shapes = grads, shapes
        ctx.inputs = tuple((t.dtype, t.device) for t in (value, reward, policy))
        ctx.mark_non_differentiable(packed)
        return packed[0].clone(), packed

    @staticmethod
    def backward(ctx, grad_loss, _grad_packed):
        if torch.is_grad_enabled():
            raise NotImplementedError("mzx.trainer.muzero_loss has no second derivative (create_graph=True)")
        gv, gr, gp = ctx.grads
        out = []
        for g, shape, (dtype, device), need in zip((gv, gr, gp), ctx.shapes + (gp.shape,), ctx.inputs, ctx.needs_input_grad[:3]):
            out.append((g * grad_loss.to(g.dtype)).reshape(shape).to(device, dtype) if need else None)
        return out[0], out[1], out[2], None, None, None


def _stacked(x):
    return torch.stack(list(x), 0) if isinstance(x, (list, tuple)) else x


def _loss_packed(value_logits, reward_logits, policy_logits, target_value, target_reward, target_policy, weight_batch,
                 gradient_scale_batch, config, backend):
    be = _backend(backend)
    targets = (_f32(be, target_value), _f32(be, target_reward), _f32(be, target_policy),
               None if weight_batch is None else _f32(be, weight_batch), _f32(be, gradient_scale_batch))
    scalars = (int(config.support_size), float(config.value_loss_weight), float(config.PER_alpha))
    return _MuZeroLoss.apply(_stacked(value_logits), _stacked(reward_logits), _stacked(policy_logits), be, targets, scalars)


def muzero_loss(value_logits, reward_logits, policy_logits, target_value, target_reward, target_policy, weight_batch,
                gradient_scale_batch, config, backend=None):
    """
    trainer.py:161-258 for the head outputs of the K + 1 unroll steps.

    ``value_logits`` / ``reward_logits`` / ``policy_logits``: step-major tensors [K + 1, batch, width] or the reference's
    lists of K + 1 per-step [batch, width] tensors (stacked here; autograd routes the gradients back to every step); a
    trailing singleton dimension on value / reward logits is accepted.  Targets as ``mzx.replay.trainer_tensors`` returns
    them: scalar ``target_value`` / ``target_reward`` [batch, K + 1], ``target_policy`` [batch, K + 1, A],
    ``weight_batch`` [batch] or None (PER off), ``gradient_scale_batch`` [batch, K + 1].  ``config`` supplies
    ``support_size``, ``value_loss_weight`` and ``PER_alpha``.

    Returns ``(loss, value_loss, reward_loss, policy_loss, priorities)``: ``loss`` a 0-d tensor with a ``grad_fn``
    (``loss.backward()`` hands the logits the gradients the reference's autograd graph gives them, gradient scales of
    the ``register_hook`` lines included), the three batch means ``update_weights`` logs as detached 0-d tensors, and
    ``priorities`` float32 [batch, K + 1] = ``|support_to_scalar(value) - target_value| ** PER_alpha``.  Everything
    stays on the device; one library call on torch's current stream, nothing synchronises.
    """
    loss, packed = _loss_packed(value_logits, reward_logits, policy_logits, target_value, target_reward, target_policy,
                                weight_batch, gradient_scale_batch, config, backend)
    return loss, packed[1], packed[2], packed[3], packed[4:].view(target_value.shape[0], -1)


def update_weights(model, optimizer, batch, config, backend=None):
    """
    ``Trainer.update_weights`` (trainer.py:124-273) with ``self`` unbound: ``batch`` is the second element of
    ``get_batch()``'s result (device tensors with a ``DeviceGameStore``, host arrays otherwise).  The prediction loop is
    the reference's, the 0.5 hook on the hidden state included; the loss head is ``muzero_loss``.  Returns the
    reference's tuple ``(priorities float32 numpy [batch, K + 1], loss, value_loss, reward_loss, policy_loss)`` after ONE
    download -- ``ReplayBuffer.update_priorities`` takes the array unchanged.  The caller advances ``training_step``.
    A ``HipNetwork`` takes the native path: ``mzx_train_fc_step`` (fully connected) or ``mzx_train_resnet_step``
    (residual) writes the gradient of its flat parameter, then ``optimizer.step()`` and ``model.refresh_derived()``; one
    the kernels do not run raises ``NotImplementedError``.
    """
    packed, batch_size = _sgd_step(model, optimizer, batch, config, backend)
    host = packed.cpu().numpy()
    priorities = host[4:].reshape(batch_size, -1)
    return priorities, float(host[0]), float(host[1]), float(host[2]), float(host[3])


def _sgd_step(model, optimizer, batch, config, backend):
    """The prediction loop, ``muzero_loss`` and one optimizer step of ``update_weights``: (packed [4 + B * steps] on the
    device -- the four losses, then the priorities --, B).  Nothing is downloaded."""
    if isinstance(model, models.HipNetwork):
        if model._cfg.network != 0:
            # parameters() is the one flat leaf, running_mean / running_var included: their gradient spans are exact
            # zeros, and the commit AFTER the optimizer step overwrites whatever it did to them (weight decay) with the
            # statistics computed from the pre-step values -- the reference never decays a buffer
            stats = {}
            packed = train_resnet_gradients(model, batch, config, stats=stats)
            # behind a downsample stem representation_network.module.conv / .bn are never applied: the reference's optimizer
            # skips them (their .grad is None), so weight decay and Adam's moments must not move them here either
            flat = model.flat_weights()
            # (a native optimizer visits neither the statistics nor the bypassed tensors: nothing to keep)
            bypassed = [(off, numel, flat[off:off + numel].clone()) for key, off, numel, _ in model._tensors
                        if key.startswith(_BYPASSED)] if model._cfg.downsample and not isinstance(optimizer, optim.NATIVE) else []
            optimizer.step()
            for off, numel, kept in bypassed:
                flat[off:off + numel].copy_(kept)
            commit_running_stats(model, stats["running"], stats["applications"])
            model.refresh_derived()
            return packed, len(batch[2])
        packed = train_fc_gradients(model, batch, config)
        optimizer.step()
        model.refresh_derived()
        return packed, len(batch[2])
    device = next(model.parameters()).device
    (observation_batch, action_batch, target_value, target_reward, target_policy, weight_batch,
     gradient_scale_batch) = replay.trainer_tensors(batch, device)
    if not config.PER:
        weight_batch = None

    value, reward, policy_logits, hidden_state = model.initial_inference(observation_batch)
    predictions = [(value, reward, policy_logits)]
    for i in range(1, action_batch.shape[1]):
        value, reward, policy_logits, hidden_state = model.recurrent_inference(hidden_state, action_batch[:, i])
        # Scale the gradient at the start of the dynamics function (See paper appendix Training)
        hidden_state.register_hook(lambda grad: grad * 0.5)
        predictions.append((value, reward, policy_logits))

    loss, packed = _loss_packed([p[0] for p in predictions], [p[1] for p in predictions], [p[2] for p in predictions],
                                target_value, target_reward, target_policy, weight_batch, gradient_scale_batch, config,
                                backend)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return packed, target_value.shape[0]


def _fc_limit(model):
    return ("residual networks train through torch (fully connected networks only)" if model._cfg.network != 0 else
            "its weights and per-wave activations exceed the 160 KiB LDS budget of the training kernels")


def _resnet_limit(model):
    cfg = model._cfg
    return ("fully connected networks train through mzx_train_fc_step (residual networks only)" if cfg.network != 1 else
            "downsample stems (the strided convolutions and pools) are not trained natively unless config.train_downsample "
            "/ HipNetwork.train_stem is set" if cfg.downsample and not model.train_stem else
            "the training kernels need at least one residual block per network" if cfg.blocks < 1 else
            "BatchNorm in training mode needs more than one value per channel (batch x board >= 2)")


# the library entries of a network kind, its io struct, and the wording of its refusal
_StepKind = collections.namedtuple("_StepKind", "name io limit")
_FC = _StepKind("mzx_train_fc", _lib.TrainFcIO, _fc_limit)
_RESNET = _StepKind("mzx_train_resnet", _lib.TrainResnetIO, _resnet_limit)
TRAIN_SCRATCH_MAX_BYTES = 32 << 30
_BYPASSED = optim._BYPASSED      # with config.downsample


def _train_gradients(kind, model, batch, config, logits, stats=None):
    """``train_fc_gradients`` / ``train_resnet_gradients``: one ``<kind.name>_step`` call.  Only the residual kind has a
    scratch ceiling, the ``d_stats`` output and the ``applications`` table."""
    be, lib = model.backend, model.backend.lib
    residual = kind is _RESNET
    (observation, action, target_value, target_reward, target_policy, weight,
     scale) = replay.trainer_tensors(batch, be.device)
    if not config.PER:
        weight = None
    batch_size, steps = target_value.shape
    if not getattr(lib, kind.name + "_supported")(model.handle, batch_size, steps):
        raise NotImplementedError(f"{kind.name}_step does not run this network at batch {batch_size} x {steps} steps: "
                                  f"{kind.limit(model)}")
    scratch_bytes = int(getattr(lib, kind.name + "_scratch_bytes")(model.handle, batch_size, steps))
    if residual:
        most = int(getattr(config, "train_scratch_max_bytes", TRAIN_SCRATCH_MAX_BYTES))
        if scratch_bytes > most:
            raise NotImplementedError(f"{kind.name}_step at batch {batch_size} x {steps} steps keeps {scratch_bytes} bytes of "
                                      f"activations, more than config.train_scratch_max_bytes = {most}")
    observation = observation.reshape(batch_size, -1).contiguous()
    actions = model.action_space_size
    if (observation.shape[1] != model.input_size or action.numel() != batch_size * steps
            or target_reward.shape != (batch_size, steps) or scale.shape != (batch_size, steps)
            or target_policy.shape != (batch_size, steps, actions) or (weight is not None and weight.shape != (batch_size,))):
        raise ValueError(f"batch: expected observation [batch, {model.input_size}], action / value / reward / gradient scale "
                         f"[batch, steps], policy [batch, steps, {actions}], weight [batch]")
    action = action.reshape(batch_size, steps).to(torch.int32).contiguous()
    tensors = [t.contiguous() for t in (target_value, target_reward, target_policy, scale)]
    param = next(model.parameters())
    if param.grad is None:
        param.grad = torch.zeros_like(model.flat_weights())
    packed = be.empty((4 + batch_size * steps,), torch.float32)
    scratch = be.empty((scratch_bytes // 4,), torch.float32)
    io = kind.io()
    io.d_flat, io.d_observation, io.d_action = model.flat_weights().data_ptr(), observation.data_ptr(), action.data_ptr()
    io.d_target_value, io.d_target_reward, io.d_target_policy, io.d_gradient_scale = (t.data_ptr() for t in tensors)
    io.d_weight = None if weight is None else weight.contiguous().data_ptr()
    io.batch, io.steps = batch_size, steps
    io.value_loss_weight, io.per_alpha = float(config.value_loss_weight), float(config.PER_alpha)
    io.d_grad_flat, io.d_losses, io.d_priorities = param.grad.data_ptr(), packed.data_ptr(), packed[4:].data_ptr()
    if logits is not None:
        width = model.full_support_size
        logits["value"], logits["reward"] = (be.empty((steps, batch_size, width), torch.float32) for _ in range(2))
        logits["policy"] = be.empty((steps, batch_size, actions), torch.float32)
        io.d_value_logits, io.d_reward_logits, io.d_policy_logits = (logits[k].data_ptr() for k in ("value", "reward", "policy"))
    io.d_scratch, io.scratch_bytes = scratch.data_ptr(), scratch_bytes
    if residual:
        running = be.empty((int(lib.mzx_train_resnet_stat_floats(model.handle)),), torch.float32)
        io.d_stats = running.data_ptr()
    lib.check(getattr(lib, kind.name + "_step")(model.handle, ctypes.byref(io), be.stream()))
    if residual and stats is not None:
        stats["running"] = running
        stats["applications"] = _applications(model, steps)
    return packed


def train_fc_gradients(model, batch, config, logits=None):
    """
    ``Trainer.update_weights`` lines 168-262 -- the unrolled predictions, the loss and ``loss.backward()`` -- for a fully
    connected ``HipNetwork`` as one ``mzx_train_fc_step`` call on the network's backend and torch's current stream.
    ``.grad`` of ``next(model.parameters())`` is OVERWRITTEN with d loss / d parameter (allocated once, then reused: no
    ``zero_grad()`` is needed).  Returns the packed device tensor [4 + B * steps]: loss, value / reward / policy loss
    means, then the priorities.  ``logits``: an optional dict that receives the step-major ``value`` / ``reward`` /
    ``policy`` logits.  Nothing synchronises.
    """
    return _train_gradients(_FC, model, batch, config, logits)


def train_resnet_gradients(model, batch, config, logits=None, stats=None):
    """
    The twin of ``train_fc_gradients`` for a residual ``HipNetwork``: ``Trainer.update_weights`` lines 168-262 in
    ``model.train()`` mode (BatchNorm on batch statistics) as one ``mzx_train_resnet_step`` call.  ``.grad`` of
    ``next(model.parameters())`` is OVERWRITTEN (exact zeros in the spans of ``running_mean`` / ``running_var``).
    Returns the packed device tensor [4 + B * steps].  ``logits``: an optional dict that receives the step-major logits.
    ``stats``: an optional dict that receives ``running`` (the packed running statistics after the step, computed from
    those in the flat buffer; ``commit_running_stats`` writes them into it) and ``applications`` (per network prefix, how
    often it was applied: what ``num_batches_tracked`` rises by; the first matching prefix counts, and the
    ``representation_network.module.bn.`` a downsample stem bypasses comes first with 0).  Nothing synchronises.  A step whose scratch exceeds
    ``config.train_scratch_max_bytes`` (default 32 GiB) raises ``NotImplementedError``.
    """
    return _train_gradients(_RESNET, model, batch, config, logits, stats)


def commit_running_stats(model, running, applications):
    """Write the running statistics of ``train_resnet_gradients`` into the flat buffer (``mzx_train_resnet_commit_stats``) and
    raise every ``num_batches_tracked`` by its network's application count.  Call ``model.refresh_derived()`` after it."""
    be, lib = model.backend, model.backend.lib
    lib.check(lib.mzx_train_resnet_commit_stats(model.handle, be.ptr(running), be.ptr(model.flat_weights()), be.stream()))
    _count_applications(model, applications)


def _applications(model, steps):
    """Per network prefix, how often a step of ``steps`` (= num_unroll_steps + 1) applies it; the first match counts."""
    table = {"representation_network.": 1, "dynamics_network.": steps - 1, "prediction_network.": steps}
    if model._cfg.downsample:      # the stem bypasses representation_network.module.conv / .bn (first match wins)
        table = {"representation_network.module.bn.": 0, **table}
    return table


def _count_applications(model, applications, times=1):
    """Raise every ``num_batches_tracked`` by ``times`` x its network's application count."""
    for key, *_ in model._tensors:
        if key.endswith(".running_var"):
            nbt = key[: -len("running_var")] + "num_batches_tracked"
            count = next(n for prefix, n in applications.items() if key.startswith(prefix))
            model._num_batches_tracked[nbt] = model._num_batches_tracked.get(nbt, torch.zeros((), dtype=torch.int64)) + times * count


def update_lr(optimizer, config, training_step):
    """``Trainer.update_lr`` (trainer.py:275-283) with ``self`` unbound."""
    lr = config.lr_init * config.lr_decay_rate ** (training_step / config.lr_decay_steps)
    for param_group in optimizer.param_groups:
        param_group["lr"] = lr


def _tensor_table(net):
    """(key, offset, numel, shape) of every tensor of the flat buffer (``mzx_net_tensor_info``) that is a PARAMETER in the
    reference: ``running_mean`` / ``running_var`` are buffers there, so index i below is the reference's ``parameters()``
    index (a fully connected network has no buffers)."""
    return [t for t in net._tensors if not t[0].endswith((".running_mean", ".running_var"))]


def optimizer_state(optimizer, net):
    """
    ``optimizer.state_dict()`` of an optimizer over ``net.parameters()`` (one flat parameter) in the form the reference's
    optimizer over ``models.MuZeroNetwork(config).parameters()`` has (trainer.py:46-67, ``copy.deepcopy(optimizer.
    state_dict())`` in a checkpoint): parameter i is tensor i of ``mzx_net_tensor_info`` (the order of the reference's
    ``parameters()``), every flat state tensor (``momentum_buffer``, ``exp_avg``, ``exp_avg_sq``, ...) is cut into
    per-tensor pieces of the parameter's shape (on the CPU), scalars and 0-d tensors (``step``) are repeated.
    """
    table = _tensor_table(net)
    flat = optimizer.state_dict()
    state = {}
    for index, entry in flat["state"].items():
        if index != 0:
            raise ValueError("optimizer_state: the optimizer must hold the network's one flat parameter")
        for i, (_, off, numel, shape) in enumerate(table):
            state[i] = {k: (v[off:off + numel].reshape(shape).detach().cpu().clone()
                            if torch.is_tensor(v) and v.dim() == 1 and v.numel() == net.num_params
                            else (v.detach().cpu().clone() if torch.is_tensor(v) else v)) for k, v in entry.items()}
    groups = []
    for group in flat["param_groups"]:
        group = dict(group)
        group["params"] = list(range(len(table)))
        groups.append(group)
    return {"state": state, "param_groups": groups}


def load_optimizer_state(optimizer, net, state_dict):
    """The inverse of ``optimizer_state``: load a reference-format optimizer ``state_dict`` (per parameter) into an
    optimizer over ``net.parameters()``."""
    table = _tensor_table(net)
    device = net.flat_weights().device
    per_param = state_dict["state"]
    flat_state = {}
    if per_param:
        if sorted(per_param) != list(range(len(table))):
            raise ValueError(f"load_optimizer_state: expected state for parameters 0 .. {len(table) - 1}")
        entry = collections.OrderedDict()
        for key, first in per_param[0].items():
            if torch.is_tensor(first) and tuple(first.shape) == tuple(table[0][3]) and first.dim() > 0:
                joined = torch.zeros(net.num_params, dtype=first.dtype, device=device)      # (the buffers' spans: no state)
                for i, (_, off, numel, shape) in enumerate(table):
                    piece = per_param[i][key]
                    if tuple(piece.shape) != tuple(shape):
                        raise ValueError(f"load_optimizer_state: {key} of parameter {i} has shape {tuple(piece.shape)}, expected {shape}")
                    joined[off:off + numel] = piece.reshape(-1).to(device)
                entry[key] = joined
            else:
                entry[key] = first.clone() if torch.is_tensor(first) else first
        flat_state[0] = entry
    groups = []
    for group in state_dict["param_groups"]:
        group = dict(group)
        group["params"] = [0]
        groups.append(group)
    optimizer.load_state_dict({"state": flat_state, "param_groups": groups})


def train_step(model, optimizer, replay_buffer, config, backend=None):
    """
    One training step as a chain of launches: ``replay_buffer.get_batch()`` (a ``mzx.replay.ReplayBuffer`` with
    ``device_sampler=True``: the batch is drawn and gathered on the device) -> the prediction loop, ``muzero_loss`` and the
    optimizer step of ``update_weights`` -> with PER ``replay_buffer.update_priorities(device priorities, index_batch)``
    (the device scatter).  Returns the four losses ``(loss, value_loss, reward_loss, policy_loss)`` as ONE packed device
    tensor [4]; nothing is downloaded and nothing synchronises.  The caller advances ``training_step``.
    """
    index_batch, batch = replay_buffer.get_batch()
    packed, batch_size = _sgd_step(model, optimizer, batch, config, backend)
    if config.PER:
        replay_buffer.update_priorities(packed[4:].view(batch_size, -1), index_batch)
    return packed[:4]


def _lr_at(config, training_step):
    return config.lr_init * config.lr_decay_rate ** (training_step / config.lr_decay_steps)


def chain_refusal(model, optimizer, replay_buffer, config):
    """What ``train_steps`` lacks to chain these four, by name, or None (``Trainer`` chooses its route with it)."""
    if not isinstance(model, models.HipNetwork):
        return "a torch model is not chained (a mzx.models.HipNetwork trains natively; use update_lr + train_step)"
    if not isinstance(optimizer, optim.NATIVE):
        return ("a torch optimizer is not chained (mzx.optim.Adam / mzx.optim.SGD run as the library's kernel; use update_lr + "
                "train_step)")
    store = getattr(replay_buffer, "_store", None)
    if not getattr(replay_buffer, "_sampler", False) or store is None or store.sampler is None:
        return ("the replay buffer has no device sampler (mzx.replay.ReplayBuffer(..., device_sampler=True) draws batches on "
                "the device)")
    lib = model.backend.lib
    cfg = replay_buffer._stock.config
    batch_size, steps = int(cfg.batch_size), int(cfg.num_unroll_steps) + 1
    kind = _RESNET if model._cfg.network != 0 else _FC
    if not lib.mzx_train_chain_supported(model.handle, batch_size, steps):
        return f"{kind.name}_step does not run this network at batch {batch_size} x {steps} steps: {kind.limit(model)}"
    nbytes = int(lib.mzx_train_chain_scratch_bytes(model.handle, batch_size, steps))
    most = int(getattr(config, "train_scratch_max_bytes", TRAIN_SCRATCH_MAX_BYTES))
    if nbytes > most:
        return (f"the chain's scratch at batch {batch_size} x {steps} steps is {nbytes} bytes, more than "
                f"config.train_scratch_max_bytes = {most}")
    return None


def train_steps(model, optimizer, replay_buffer, config, n, training_step):
    """
    ``n`` whole training steps queued by ONE library call (``mzx_train_chain``, csrc/mzx_train_chain.h).  By definition

        for i in range(n):
            update_lr(optimizer, config, training_step + i)
            losses[i] = train_step(model, optimizer, replay_buffer, config)

    and it leaves, bit for bit, what that loop leaves: the flat weights and the derived buffer, every optimizer state
    tensor, ``state["step"]`` and ``param_groups[0]["lr"]`` (those of the last step), the store's priorities,
    ``replay_buffer._sample_calls`` (advanced by ``n``) and every ``num_batches_tracked``.  Returns the losses as a device
    tensor [n, 4] (loss, value / reward / policy loss per step); nothing is downloaded and nothing synchronises.  The
    caller advances ``training_step``, as with ``train_step``.

    Per step the library queues the sampler's draw (call counter ``_sample_calls + i``; ``total_samples`` and the slot
    table as flushed once before the chain), the gather, the conversions ``trainer_tensors`` makes with torch, the native
    step, the native optimizer's launch, for a residual network the commit of the running statistics and with PER the
    priority scatter.  The BatchNorm re-fold (``mzx_net_set_weights``) runs ONCE, behind the last step: the training kernels
    read the flat buffer, not the derived one -- a search running beside the chain sees folded terms at chunk granularity.
    The per-step scalars (lr, Adam's step size and bias correction) are computed here in binary64, as torch computes
    them.  The one workspace (``mzx_train_chain_scratch_bytes``) is allocated once per (network, batch, steps) and kept on
    the network.

    There is no fall-back: a torch optimizer, a torch model, a buffer without ``device_sampler=True``, a network the
    native step refuses and a workspace above ``config.train_scratch_max_bytes`` raise ``NotImplementedError`` by name
    before anything is queued; ``n < 1`` raises ``ValueError``.
    """
    n = int(n)
    if n < 1:
        raise ValueError(f"train_steps: n = {n}, at least one step")
    missing = chain_refusal(model, optimizer, replay_buffer, config)
    if missing:
        raise NotImplementedError("train_steps: " + missing)
    store = replay_buffer._store
    be, lib = model.backend, model.backend.lib
    cfg = replay_buffer._stock.config
    if bool(cfg.PER) != bool(config.PER):
        raise ValueError("train_steps: config.PER differs from the replay buffer's")
    batch_size, steps = int(cfg.batch_size), int(cfg.num_unroll_steps) + 1
    kind = _RESNET if model._cfg.network != 0 else _FC
    nbytes = int(lib.mzx_train_chain_scratch_bytes(model.handle, batch_size, steps))
    if tuple(store.sample_shape) != tuple(model.input_shape) and int(numpy.prod(store.sample_shape)) != model.input_size:
        raise ValueError("train_steps: the store's stacked observation is not the network's input")
    if not store._with_positions:
        raise ValueError("no game with a position is resident: nothing to draw from")
    param = next(model.parameters())
    if param.grad is None:
        param.grad = torch.zeros_like(model.flat_weights())
    io = _lib.TrainChainIO()
    group, _, _, oio = optimizer._io(_lib.OPTIM_ADAM if isinstance(optimizer, optim.Adam) else _lib.OPTIM_SGD,
                                     type(optimizer).__name__, optimizer._REFUSED)
    lrs = [_lr_at(config, training_step + i) for i in range(n)]
    h_lr = numpy.array(lrs, dtype=numpy.float64)
    keep = [h_lr]
    if isinstance(optimizer, optim.Adam):
        step, exp_avg, exp_avg_sq = optimizer.native_state()
        first_t = int(step.item()) + 1
        beta1, beta2 = group["betas"]
        oio.t, oio.d_state1, oio.d_state2 = first_t, exp_avg.data_ptr(), exp_avg_sq.data_ptr()
        oio.one_minus_beta1, oio.beta2, oio.one_minus_beta2, oio.eps = 1 - beta1, beta2, 1 - beta2, group["eps"]
        scalars = numpy.array([optimizer.adam_scalars(first_t + i, lrs[i]) for i in range(n)], dtype=numpy.float64)
        h_ss, h_bc = numpy.ascontiguousarray(scalars[:, 0]), numpy.ascontiguousarray(scalars[:, 1])
        keep += [h_ss, h_bc]
        io.h_step_size, io.h_bias_correction2_sqrt = h_ss.ctypes.data, h_bc.ctypes.data
    else:
        step = None
        oio.t, oio.momentum = 1, float(group["momentum"])
        if group["momentum"] != 0:
            buf, first = optimizer.native_state()
            oio.d_state1, oio.first_step = buf.data_ptr(), int(first)
        io.h_lr = h_lr.ctypes.data
    io.optim = oio
    # the sampler's state as get_batch() leaves it before a draw (DeviceGameStore.sample)
    store._flush_slots()
    if cfg.PER and store._raw.numel() < batch_size:
        store._raw = be.empty((batch_size,), torch.float64)
        store.sampler.d_raw, store.sampler.raw_capacity = store._raw.data_ptr(), batch_size
    io.pool, io.sampler = ctypes.pointer(store.pool), ctypes.pointer(store.sampler)
    io.seed, io.first_call = int(cfg.seed) & (2 ** 64 - 1), int(replay_buffer._sample_calls) & (2 ** 64 - 1)
    io.total_samples, io.per, io.num_unroll_steps = int(replay_buffer._stock.total_samples), int(bool(cfg.PER)), steps - 1
    io.stacked_observations, io.num_actions = store.k, store.A
    io.d_action_space = None if store._action_space is None else store._action_space.data_ptr()
    io.batch, io.num_steps = batch_size, n
    io.value_loss_weight, io.per_alpha = float(config.value_loss_weight), float(config.PER_alpha)
    io.d_flat, io.d_grad_flat = model.flat_weights().data_ptr(), param.grad.data_ptr()
    losses = be.empty((n, 4), torch.float32)
    io.d_losses = losses.data_ptr()
    io.d_derived, io.derived_floats = model._derived.data_ptr(), model._derived.numel()
    key = (batch_size, steps)
    workspace = getattr(model, "_chain_workspace", None)
    if workspace is None or workspace[0] != key:
        workspace = model._chain_workspace = (key, be.empty((nbytes + 256,), torch.uint8))
    offset = -workspace[1].data_ptr() % 256
    io.d_workspace, io.workspace_bytes = workspace[1].data_ptr() + offset, nbytes
    lib.check(lib.mzx_train_chain(model.handle, ctypes.byref(io), be.stream()))
    if step is not None:
        step.fill_(float(first_t + n - 1))
    group["lr"] = lrs[-1]
    replay_buffer._sample_calls = replay_buffer._sample_calls + n
    if kind is _RESNET:
        _count_applications(model, _applications(model, steps), n)
    return losses


class Trainer:
    """
    trainer.py:13-123 -- the worker that trains the network and publishes it in the shared storage, under the reference's
    names: ``Trainer(initial_checkpoint, config)``, ``continuous_update_weights(replay_buffer, shared_storage)``,
    ``update_weights(batch)``, ``update_lr()``.  The network is ``models.MuZeroNetwork(config)``, the optimizer
    ``mzx.optim.from_config`` (the library's kernel), the optimizer state travels in the reference's per-parameter format
    (``optimizer_state`` / ``load_optimizer_state``).  ``_backend``: the serial build, for the tests.

    The loop trains in chunks of ``min(config.train_steps_chunk (default 16), steps to the next multiple of
    checkpoint_interval, steps left)``: one ``train_steps`` call and one download of the chunk's [chunk, 4] losses; then the
    storage traffic of the reference's loop -- weights and optimizer state at every multiple of ``checkpoint_interval``,
    the six logged entries (the last step's losses), ``training_delay``, the ``ratio`` wait, ``terminate``.  With
    ``train_steps_chunk = 1`` the storage sees exactly the reference's sequence of ``set_info`` calls.  What ``train_steps``
    refuses (``chain_refusal``) takes a per-step route, chosen once at the first chunk and readable as ``route``: "chain",
    "step" (``update_lr`` + ``train_step`` with a device sampler) or "host" (``get_batch`` / ``update_weights`` /
    ``update_priorities`` through the buffer's own methods, a Ray actor's included).
    """

    def __init__(self, initial_checkpoint, config, _backend=None):
        self.config = config
        # Fix random generator seed (trainer.py:21-23)
        numpy.random.seed(self.config.seed)
        torch.manual_seed(self.config.seed)
        # the network lives on the GPU whatever config.train_on_gpu says: the engine has no CPU path
        self.model = models.MuZeroNetwork(self.config, _backend=_backend)
        self.model.set_weights(copy.deepcopy(initial_checkpoint["weights"]))
        self.model.train()
        self.training_step = initial_checkpoint["training_step"]
        if "cuda" not in str(next(self.model.parameters()).device):
            print("You are not training on GPU.\n")
        self.optimizer = optim.from_config(self.model, self.config)
        if initial_checkpoint["optimizer_state"] is not None:
            print("Loading optimizer...\n")
            load_optimizer_state(self.optimizer, self.model, copy.deepcopy(initial_checkpoint["optimizer_state"]))
        self.route = None      # chosen at the first chunk of continuous_update_weights
        self._backend = _backend

    def _choose_route(self, replay_buffer):
        self.route_reason = chain_refusal(self.model, self.optimizer, replay_buffer, self.config)
        if self.route_reason is None:
            return "chain"
        return "step" if getattr(replay_buffer, "_sampler", False) else "host"

    def _optimizer_state(self):
        if isinstance(self.model, models.HipNetwork):
            return optimizer_state(self.optimizer, self.model)
        return copy.deepcopy(models.dict_to_cpu(self.optimizer.state_dict()))

    def _train_chunk(self, replay_buffer, chunk):
        """``chunk`` steps on the chosen route -> the last step's four losses as floats, after one download."""
        if self.route == "chain":
            losses = train_steps(self.model, self.optimizer, replay_buffer, self.config, chunk, self.training_step)
            self.training_step += chunk
            return [float(x) for x in losses.cpu().numpy()[-1]]
        if self.route == "step":
            for _ in range(chunk):
                self.update_lr()
                packed = train_step(self.model, self.optimizer, replay_buffer, self.config, backend=self._backend)
                self.training_step += 1
            return [float(x) for x in packed.cpu().numpy()]
        for _ in range(chunk):
            index_batch, batch = _remote(replay_buffer.get_batch)
            self.update_lr()
            priorities, *last = self.update_weights(batch)
            if self.config.PER:
                # Save new priorities in the replay buffer (See https://arxiv.org/abs/1803.00933)
                _remote(replay_buffer.update_priorities, priorities, index_batch)
        return last

    def continuous_update_weights(self, replay_buffer, shared_storage):
        cfg = self.config
        # Wait for the replay buffer to be filled
        while _remote(shared_storage.get_info, "num_played_games") < 1:
            time.sleep(0.1)
        # Training loop
        while self.training_step < cfg.training_steps and not _remote(shared_storage.get_info, "terminate"):
            if self.route is None:
                self.route = self._choose_route(replay_buffer)
            interval = int(cfg.checkpoint_interval)
            chunk = min(max(1, int(getattr(cfg, "train_steps_chunk", 16))), interval - self.training_step % interval,
                        cfg.training_steps - self.training_step)
            total_loss, value_loss, reward_loss, policy_loss = self._train_chunk(replay_buffer, chunk)
            # Save to the shared storage
            if self.training_step % interval == 0:
                _remote(shared_storage.set_info, {"weights": copy.deepcopy(self.model.get_weights()),
                                                  "optimizer_state": self._optimizer_state()})
                if cfg.save_model:
                    _remote(shared_storage.save_checkpoint)
            _remote(shared_storage.set_info, {
                "training_step": self.training_step,
                "lr": self.optimizer.param_groups[0]["lr"],
                "total_loss": total_loss,
                "value_loss": value_loss,
                "reward_loss": reward_loss,
                "policy_loss": policy_loss,
            })
            # Managing the self-play / training ratio
            if cfg.training_delay:
                time.sleep(cfg.training_delay)
            if cfg.ratio:
                while (self.training_step / max(1, _remote(shared_storage.get_info, "num_played_steps")) > cfg.ratio
                       and self.training_step < cfg.training_steps
                       and not _remote(shared_storage.get_info, "terminate")):
                    time.sleep(0.5)

    def update_weights(self, batch):
        """One training step on ``batch`` (trainer.py:124-273): ``(priorities, total_loss, value_loss, reward_loss,
        policy_loss)``; ``training_step`` advances."""
        out = update_weights(self.model, self.optimizer, batch, self.config, backend=self._backend)
        self.training_step += 1
        return out

    def update_lr(self):
        """trainer.py:275-283"""
        update_lr(self.optimizer, self.config, self.training_step)
