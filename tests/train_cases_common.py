"""
What the case modules and tests of the two native trainers share (fc_train_cases, resnet_train_cases,
resnet_stem_train_cases; test_{,gpu_}{fc,resnet,resnet_stem}_train.py; the bit fixtures): the torch pieces of the
restatements, the seeded batch, the common part of ``run_native``, the io struct of a step over tensors pre-filled with 7,
and the checks that do not depend on the network kind.  ``kind`` is "fc" or "resnet": which of mzx_train_fc_step /
mzx_train_resnet_step is meant; ``tables`` is the case module a check runs on.
"""
import ctypes
import importlib.util
import os

import numpy
import torch

from mzx import _lib


def _mlp(sizes):
    """models.mlp: Linear + ELU per hidden layer, Linear + identity at the end."""
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        layers.append(torch.nn.ELU() if i < len(sizes) - 2 else torch.nn.Identity())
    return torch.nn.Sequential(*layers)


def _unit_range(state, dim):
    """The reference's min-max normalisation of a state over its dimensions from ``dim`` on (1: a fully connected
    encoding, 2: the board of every channel)."""
    flat = state.flatten(dim)
    keep = flat.shape[:dim] + (1,) * (state.dim() - dim)
    low = flat.min(dim, keepdim=True)[0].reshape(keep)
    high = flat.max(dim, keepdim=True)[0].reshape(keep)
    span = high - low
    span[span < 1e-5] += 1e-5
    return (state - low) / span


def load(module, state, strict=True):
    module.load_state_dict({k: torch.from_numpy(numpy.ascontiguousarray(v)) for k, v in state.items()}, strict=strict)
    return module


def input_channels(case):
    return case["obs"][0] * (case["stacked"] + 1) + case["stacked"]


def batch(case):
    """A host batch in the layout of ``get_batch()``'s second element (observation, action, target value / reward /
    policy, PER weight or None, gradient scale)."""
    B, steps, A = case["B"], case["steps"], case["A"]
    _, h, w = case["obs"]
    rs = numpy.random.RandomState(case["seed"])
    observation = rs.standard_normal((B, input_channels(case), h, w)).astype(numpy.float32)
    action = rs.randint(0, A, size=(B, steps)).astype(numpy.int64)
    tv = (rs.standard_normal((B, steps)) * 4).astype(numpy.float32)
    tr = (rs.standard_normal((B, steps)) * 2).astype(numpy.float32)
    tp = rs.dirichlet(numpy.ones(A) * 0.7, size=(B, steps)).astype(numpy.float32)
    K = max(steps - 1, 1)
    scale = numpy.repeat((1 + numpy.arange(B) % K).astype(numpy.float32)[:, None], steps, 1)   # 1 .. K, one per sample
    weight = (0.1 + 0.9 * rs.random_sample(B)).astype(numpy.float32) if case["per"] else None
    return (observation, action, tv, tr, tp, weight, numpy.ascontiguousarray(scale))


def is_statistic(key):
    return key.endswith((".running_mean", ".running_var"))


def adam_reference_step(net, grad_flat, flat_before, **hp):
    """torch Adam applied PER TENSOR to the parameters (not the running statistics) of the flat gradient split by
    mzx_net_tensor_info -> {key: tensor after}."""
    params, keys = [], []
    for key, off, numel, shape in net._tensors:
        if is_statistic(key):
            continue
        p = torch.nn.Parameter(flat_before[off:off + numel].reshape(shape).clone())
        p.grad = grad_flat[off:off + numel].reshape(shape).clone()
        params.append(p), keys.append(key)
    torch.optim.Adam(params, **hp).step()
    return {k: p.detach() for k, p in zip(keys, params)}


def run_native(net, case, gradients):
    """``gradients(logits)`` is one of mzx.trainer.train_{fc,resnet}_gradients on ``net``, bound to its batch -> dict of host
    arrays: loss, value_loss, reward_loss, policy_loss, priorities, value / reward / policy logits (step-major), grad_flat and
    grad/<key> per tensor.  The gradient buffer is pre-filled with NaN: the call has to overwrite all of it."""
    param = next(net.parameters())
    param.grad = torch.full_like(net.flat_weights(), float("nan"))
    logits = {}
    host = gradients(logits).cpu().numpy()
    out = dict(loss=host[0], value_loss=host[1], reward_loss=host[2], policy_loss=host[3],
               priorities=host[4:].reshape(case["B"], case["steps"]).copy(),
               value_logits=logits["value"].cpu().numpy(), reward_logits=logits["reward"].cpu().numpy(),
               policy_logits=logits["policy"].cpu().numpy(), grad_flat=param.grad.cpu().numpy().copy())
    for key, off, numel, shape in net._tensors:
        out["grad/" + key] = out["grad_flat"][off:off + numel].reshape(shape)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The ABI of a step: a complete io struct, and what every refusal has to look like.

REQUIRED = ("d_flat", "d_observation", "d_action", "d_target_value", "d_target_reward", "d_target_policy", "d_gradient_scale",
            "d_grad_flat", "d_losses", "d_priorities", "d_scratch")
OUTPUTS = {"fc": ("grad", "losses", "priorities", "scratch"), "resnet": ("grad", "losses", "priorities", "scratch", "stats")}


def step_io(be, case, net, keep, kind, device="cpu", fill=7.0, whole=False):
    """A complete mzx_train_fc_io / mzx_train_resnet_io over tensors on ``device``, outputs pre-filled with 7 -> (io, the
    tensors by name; ``keep`` holds them alive).  ``fill``: the number the outputs and the scratch start from, or a function
    ``fill(name, tensor)`` that fills each of them in place on ``device`` (tests/poison_cases.py).  ``whole``: also the
    optional members of the struct -- the three logit outputs and, for a case with PER, the weights."""
    observation, action, tv, tr, tp, weight, scale = batch(case)
    B, steps = case["B"], case["steps"]
    nbytes = int(getattr(be.lib, f"mzx_train_{kind}_scratch_bytes")(net.handle, B, steps))
    assert nbytes > 0
    number = 7.0 if callable(fill) else fill
    t = dict(observation=torch.from_numpy(observation).reshape(B, -1).contiguous(), action=torch.from_numpy(action).to(torch.int32),
             tv=torch.from_numpy(tv), tr=torch.from_numpy(tr), tp=torch.from_numpy(tp), scale=torch.from_numpy(scale),
             grad=torch.full((net.num_params,), number), losses=torch.full((4,), number), priorities=torch.full((B, steps), number),
             scratch=torch.full((nbytes // 4,), number))
    if kind == "resnet":
        t["stats"] = torch.full((int(be.lib.mzx_train_resnet_stat_floats(net.handle)),), number)
    filled = OUTPUTS[kind]
    if whole:
        width = net.full_support_size
        t.update(value_logits=torch.full((steps, B, width), number), reward_logits=torch.full((steps, B, width), number),
                 policy_logits=torch.full((steps, B, case["A"]), number))
        filled = filled + ("value_logits", "reward_logits", "policy_logits")
        if weight is not None:
            t["weight"] = torch.from_numpy(weight)
    t = {k: v.to(device) for k, v in t.items()}
    if callable(fill):
        for key in filled:
            fill(key, t[key])
    keep.append(t)
    io = _lib.TrainFcIO() if kind == "fc" else _lib.TrainResnetIO()
    io.d_flat, io.d_observation, io.d_action = net.flat_weights().data_ptr(), t["observation"].data_ptr(), t["action"].data_ptr()
    io.d_target_value, io.d_target_reward, io.d_target_policy = t["tv"].data_ptr(), t["tr"].data_ptr(), t["tp"].data_ptr()
    io.d_gradient_scale = t["scale"].data_ptr()
    io.batch, io.steps, io.value_loss_weight, io.per_alpha = B, steps, case["vlw"], case["alpha"]
    io.d_grad_flat, io.d_losses, io.d_priorities = t["grad"].data_ptr(), t["losses"].data_ptr(), t["priorities"].data_ptr()
    io.d_scratch, io.scratch_bytes = t["scratch"].data_ptr(), nbytes
    if kind == "resnet":
        io.d_stats = t["stats"].data_ptr()
    if whole:
        io.d_value_logits, io.d_reward_logits, io.d_policy_logits = (t[k + "_logits"].data_ptr() for k in ("value", "reward", "policy"))
        io.d_weight = t["weight"].data_ptr() if "weight" in t else None
    return io, t


def check_abi_refusal(be, kind, tables, case, field, value, device="cpu", sync=lambda: None, others=()):
    """The step with ``field`` set to ``value`` ("misaligned": a d_scratch four bytes off) returns MZX_ERR_INVALID with an
    error text and launches nothing (every output still 7), from the case's network and from each network of ``others``;
    the untouched struct then runs and overwrites the outputs."""
    step = getattr(be.lib, f"mzx_train_{kind}_step")
    keep = []
    net = tables.network(be, case)
    io, t = step_io(be, case, net, keep, kind, device)
    setattr(io, field, t["scratch"].data_ptr() + 4 if value == "misaligned" else value)
    for refusing in (net,) + tuple(others):
        assert step(refusing.handle, ctypes.byref(io), be.stream()) == -1        # MZX_ERR_INVALID
        assert be.lib.mzx_last_error()
    sync()
    for key in OUTPUTS[kind]:                                                      # nothing was launched
        assert (t[key] == 7.0).all(), key
    io, t = step_io(be, case, net, keep, kind, device)
    assert step(net.handle, ctypes.byref(io), be.stream()) == 0
    sync()
    for key in OUTPUTS[kind]:
        assert key in ("priorities", "scratch") or not (t[key] == 7.0).any(), key
    return net


# ---------------------------------------------------------------------------------------------------------------------
# The optimizer over the one flat parameter.

def check_adam_bit_for_bit(be, tables, case):
    """Adam over the one flat parameter is Adam per tensor on the parameter spans, bit for bit; the spans of the running
    statistics (a residual network's) hold what the step committed, whatever Adam did to them."""
    from mzx import trainer
    hp = dict(lr=0.02, weight_decay=1e-4)
    net = tables.network(be, case)
    before = net.flat_weights().clone()
    optimizer = torch.optim.Adam(net.parameters(), **hp)
    trainer.update_weights(net, optimizer, tables.batch(case), tables.config_of(case))
    want = adam_reference_step(net, next(net.parameters()).grad, before, **hp)
    state = net.state_dict()
    committed = tables.run_native(be, case, tables.network(be, case)) if len(want) < len(net._tensors) else {}
    for key, off, numel, shape in net._tensors:
        got = state[key].cpu().numpy()
        if is_statistic(key):
            assert numpy.array_equal(got.view(numpy.int32), committed["stat/" + key].view(numpy.int32)), key
        else:
            assert not torch.equal(state[key].cpu(), before[off:off + numel].reshape(shape).cpu()), key
            assert numpy.array_equal(got.view(numpy.int32), want[key].cpu().numpy().view(numpy.int32)), key


def check_optimizer_state_round_trip(be, tables, case, make, table_of):
    """``table_of(net)``: the (key, offset, numel, shape) rows that are parameters in the reference, in its order."""
    from mzx import trainer
    net = tables.network(be, case)
    optimizer = make(net.parameters())
    for _ in range(2):
        trainer.update_weights(net, optimizer, tables.batch(case), tables.config_of(case))
    state = trainer.optimizer_state(optimizer, net)
    table = table_of(net)
    assert sorted(state["state"]) == list(range(len(table)))
    assert state["param_groups"][0]["params"] == list(range(len(table)))
    for i, (_, _, _, shape) in enumerate(table):
        for value in state["state"][i].values():
            assert not torch.is_tensor(value) or value.dim() == 0 or tuple(value.shape) == tuple(shape)
    twin_net = tables.network(be, case)
    twin = make(twin_net.parameters())
    trainer.load_optimizer_state(twin, twin_net, state)
    again = trainer.optimizer_state(twin, twin_net)
    assert again["param_groups"] == state["param_groups"] and sorted(again["state"]) == sorted(state["state"])
    for i in state["state"]:
        assert list(again["state"][i]) == list(state["state"][i])
        for key, value in state["state"][i].items():
            other = again["state"][i][key]
            assert torch.equal(value, other) if torch.is_tensor(value) else value == other, (i, key)
    return state


# ---------------------------------------------------------------------------------------------------------------------
# The bit fixtures (muzero-general_amd/tools/make_resnet_train_bits.py).

_spec = importlib.util.spec_from_file_location("make_resnet_train_bits", os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "muzero-general_amd", "tools", "make_resnet_train_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


def check_bits(be, case, tables, section, family):
    """The digests of the case's outputs are the section's; the assertion names the first output that differs."""
    want = section["cases"][case["name"]]
    pinned = bits.FAMILIES[family]["pinned"]
    assert sorted(want) == sorted(pinned)
    have = bits.digests(tables.run_native(be, case), family)
    differs = [key for key in pinned if have[key] != want[key]]
    assert not differs, f"{case['name']}: {differs[0]} differs from the bits recorded at {section['commit']} (all: {differs})"


# ---------------------------------------------------------------------------------------------------------------------
# The gates of a step against a reference run, for both network kinds (fc_train_cases / resnet_train_cases pass their own
# floor and head gate; ``tables`` is the case module: batch, weights, tensor_shapes, is_bypassed, LOSS_KEYS and, where a
# case has them, amplified).

# A tensor whose gradient a `tiny_range` recipe amplifies (``tables.amplified(case)``): the state is divided by range + 1e-5
# with range << 1e-5, so the gradient of the layer that produces it is 1e5 times the gradient of the state -- values of order
# 1e3 to 1e4, of which any float32 run gets a handful of units in the last place wrong: absolute errors of 1e-3, far above
# the absolute floor, and the reference's own float32 error there is a draw from the same noise (zero when it rounds
# luckily), no yardstick on its own.  For such a tensor the absolute floor is replaced by one from the precision of the
# format: AMPLIFIED_ULPS float32 units in the last place of its largest element -- the sum runs over at most 81 rows x positions here, each term a chain of about ten
# rounded operations behind the division, and rounding errors of such a sum grow with the square root of their number:
# sqrt(81 x 10) = 28 half-units, rounded up to a power of two.  A threshold of 1e-7 in place of 1e-5 moves these gradients
# by their own size, thousands of times this gate.
AMPLIFIED_ULPS = 32


def check_against(case, got, want32_logits, ref64, ref_errors, f32_losses, f32_pred, be, report, tables, floor, logit_gate):
    """The gates of one case.  ``ref64``: key -> binary64 arrays (losses, grad/<key>, stat/<key>); ``ref_errors``: key ->
    the reference's own float32 error against binary64 on that tensor."""
    import trainer_loss_cases
    name = case["name"]
    failures = []
    for head in ("value", "reward", "policy"):
        ours, ref = got[f"{head}_logits"], want32_logits[head]
        assert ours.shape == ref.shape, (head, ours.shape, ref.shape)
        finite = numpy.isfinite(ref)
        assert numpy.array_equal(ours[~finite], ref[~finite]), head
        err = float(numpy.max(numpy.abs(ours[finite].astype(numpy.float64) - ref[finite]))) if finite.any() else 0.0
        report(f"{name} {head} logits: error {err:.3e} against the reference float32, gate {logit_gate:.1e}")
        if not err <= logit_gate:
            failures.append(head)
    for key in tables.LOSS_KEYS:
        mine, ref = abs(float(got[key]) - float(ref64[key])), abs(float(f32_losses[key]) - float(ref64[key]))
        gate = max(4 * ref, trainer_loss_cases.LOSS_ERROR_FLOOR)
        report(f"{name} {key}: error {mine:.3e}, reference float32 error {ref:.3e}, gate {gate:.3e}")
        if not mine <= gate:
            failures.append(key)
    logits = torch.from_numpy(got["value_logits"]).to(be.device).reshape(-1, 2 * case["S"] + 1)
    pred = be.empty((logits.shape[0],), torch.float32)
    be.lib.check(be.lib.mzx_support_to_scalar(be.ptr(logits), logits.shape[0], case["S"], be.ptr(pred), be.stream()))
    pred = pred.cpu().numpy().reshape(case["steps"], case["B"]).T.copy()
    want = numpy.abs(pred - tables.batch(case)[2]) ** case["alpha"]
    assert want.dtype == numpy.float32
    ulps = trainer_loss_cases.ulp_distance(want, got["priorities"])
    report(f"{name} priorities: max ulp distance {ulps.max()} (alpha {case['alpha']})")
    assert ulps.max() <= (0 if case["alpha"] == 1.0 else 1)
    gap = numpy.abs(pred.astype(numpy.float64) - f32_pred)
    report(f"{name} decoded value against the reference: {gap.max():.3e} (values up to {numpy.abs(pred).max():.2f})")
    assert gap.max() <= trainer_loss_cases.DECODED_SCALAR_GATE
    assert not numpy.isnan(got["grad_flat"]).any(), "d_grad_flat was not fully overwritten"
    state = tables.weights(case)
    amplified = tables.amplified(case) if hasattr(tables, "amplified") else ()
    worst = (0.0, None)
    for key in tables.tensor_shapes(case):
        if is_statistic(key):
            assert numpy.array_equal(got["grad/" + key], numpy.zeros_like(got["grad/" + key])), key      # exact zeros
            kind, mine64 = "stat", got["stat/" + key]
        else:
            kind, mine64 = "grad", got["grad/" + key]
        if tables.is_bypassed(key):        # never applied: exact-zero gradients, the statistics keep their bits
            assert numpy.array_equal(got["grad/" + key], numpy.zeros_like(got["grad/" + key])), key
            if is_statistic(key):
                assert numpy.array_equal(got["stat/" + key].view(numpy.int32), state[key].reshape(-1).view(numpy.int32)), key
        ref = float(ref_errors[f"{kind}/{key}"])
        want64 = numpy.asarray(ref64[f"{kind}/{key}"]).reshape(-1)
        gate = max(4 * ref, floor)
        mine = float(numpy.max(numpy.abs(mine64.astype(numpy.float64).reshape(-1) - want64)))
        if kind == "grad" and key in amplified:
            gate = max(gate, AMPLIFIED_ULPS * 2.0 ** -23 * float(numpy.abs(want64).max()))
            report(f"{name} grad {key}: error {mine:.3e}, reference float32 error {ref:.3e}, largest element "
                   f"{numpy.abs(want64).max():.3e}, gate {gate:.3e} (floor: {AMPLIFIED_ULPS} units in its last place; amplified by 1 / 1e-5)")
        else:
            report(f"{name} {kind} {key}: error {mine:.3e}, reference float32 error {ref:.3e}, gate {gate:.3e}")
            if 4 * ref < floor and mine > worst[0]:
                worst = (mine, key)
        if not mine <= gate:
            failures.append(key)
    report(f"{name} largest error on a tensor that needs the floor: {worst[0]:.3e} ({worst[1]})")
    assert not failures, failures
