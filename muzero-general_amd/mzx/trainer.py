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
"""
import ctypes

import torch

from . import _lib, replay


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
    """
    packed, batch_size = _sgd_step(model, optimizer, batch, config, backend)
    host = packed.cpu().numpy()
    priorities = host[4:].reshape(batch_size, -1)
    return priorities, float(host[0]), float(host[1]), float(host[2]), float(host[3])


def _sgd_step(model, optimizer, batch, config, backend):
    """The prediction loop, ``muzero_loss`` and one optimizer step of ``update_weights``: (packed [4 + B * steps] on the
    device -- the four losses, then the priorities --, B).  Nothing is downloaded."""
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
