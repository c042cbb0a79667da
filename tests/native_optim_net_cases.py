"""
``mzx.optim.Adam`` / ``mzx.optim.SGD`` on networks, for the serial build (tests/test_native_optim_networks.py) and the
device (tests/test_gpu_native_optim_networks.py): the checks both run, on the cases of fc_train_cases,
resnet_train_cases and resnet_stem_train_cases (imported, unchanged) and the restatement of tests/optim_cases.py.

The yardstick against torch is the one of tests/optim_cases.py, per run: an optimizer's error is the largest absolute
distance of the parameters it leaves from ``torch.optim`` in binary64 on the CPU fed the SAME start, state and gradients
that run saw (the gradients are the native step's float32 ``.grad``, recorded step by step; the two runs' second
gradients differ in their last bits because their parameters do).  The native optimizer's error may be at most 4 x the
error of torch's float32 optimizer over the same network.  Both are computed at run time and printed.
"""
import numpy
import pytest
import torch

import fc_train_cases
import optim_cases
import resnet_stem_train_cases
import resnet_train_cases
import train_cases_common as common
from mzx import optim, trainer

ADAM_HP = dict(lr=0.02, weight_decay=1e-4)
SGD_HP = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
FC_CASE = fc_train_cases.BY_NAME["b5_k4_stacked"]
RESNET_CASE = resnet_train_cases.BY_NAME["b_b3_k3"]
STEM_CASES = [resnet_stem_train_cases.BY_NAME["sa_b2_k1"], resnet_stem_train_cases.BY_NAME["ca_b2_k2"]]
F32 = numpy.float32


def make(kind, native, **hp):
    module = optim if native else torch.optim
    if kind == "adam":
        return lambda params: module.Adam(params, **{**ADAM_HP, **hp})
    return lambda params: module.SGD(params, **{**SGD_HP, **hp})


def host(t):
    return t.detach().cpu().numpy().copy()


def state_arrays(optimizer, kind, n):
    """(first state array, second or None) of the flat parameter as host arrays; zeros before the first step."""
    state = optimizer.state_dict()["state"].get(0, {})
    keys = ("exp_avg", "exp_avg_sq") if kind == "adam" else ("momentum_buffer",)
    out = [host(state[k]) if state.get(k) is not None else numpy.zeros(n, F32) for k in keys]
    return out + [None] * (2 - len(out))


def restated_step(kind, hp, t, p, g, s1, s2):
    """One step of the definition (tests/optim_cases.py) on whole arrays -> (p, s1, s2)."""
    if kind == "adam":
        row = dict(optim_cases.ADAM, wd=hp["weight_decay"], lr=hp["lr"])
        return optim_cases.adam_restated(p, g, s1, s2, optim_cases.adam_scalars(row, t=t))
    row = dict(wd=hp["weight_decay"], mu=hp["momentum"], lr=hp["lr"], first=t == 1)
    return optim_cases.sgd_restated(p, g, s1, row) + (None,)


def steps_with_record(tables, be, case, kind, native, steps, hp=None, check_bits=False):
    """``steps`` x ``update_weights`` on a fresh network -> (net, optimizer, start, the per-step gradients).  ``check_bits``:
    after every step the live spans of the parameter and of the state equal the restatement applied to that step's
    ``.grad``, bit for bit, and nothing else moved but the statistics."""
    hp = {**(ADAM_HP if kind == "adam" else SGD_HP), **(hp or {})}
    net = tables.network(be, case)
    optimizer = make(kind, native, **hp)(net.parameters())
    n = net.num_params
    mask = optim_cases.live_mask(n, optim.live_spans(net))
    start, grads = host(net.flat_weights()), []
    for t in range(1, steps + 1):
        before = host(net.flat_weights())
        s1, s2 = state_arrays(optimizer, kind, n)
        trainer.update_weights(net, optimizer, tables.batch(case), tables.config_of(case))
        grads.append(host(next(net.parameters()).grad))
        if check_bits:
            want = restated_step(kind, hp, t, before, grads[-1], s1, s2)
            got = (host(net.flat_weights()),) + tuple(state_arrays(optimizer, kind, n))
            for name, a, b in zip(("parameter", "state 1", "state 2"), got, want):
                if b is not None:
                    assert numpy.array_equal(optim_cases.bits(a)[mask], optim_cases.bits(b)[mask]), (t, name)
            assert (got[0][mask] != before[mask]).any()
    return net, optimizer, start, grads


def binary64_run(kind, hp, start, grads, state=None, first_t=1):
    """``torch.optim`` in binary64 on the CPU over one flat parameter: ``start`` (float32 values), the recorded gradients,
    optionally a starting state (float32 arrays) -> the parameters after, binary64."""
    param = torch.nn.Parameter(torch.from_numpy(start).double())
    optimizer = (torch.optim.Adam if kind == "adam" else torch.optim.SGD)([param], **hp)
    if state is not None:
        if kind == "adam":
            optimizer.state[param] = dict(step=torch.tensor(float(first_t - 1)), exp_avg=torch.from_numpy(state[0]).double(),
                                          exp_avg_sq=torch.from_numpy(state[1]).double())
        else:
            optimizer.state[param] = dict(momentum_buffer=torch.from_numpy(state[0]).double())
    for g in grads:
        param.grad = torch.from_numpy(g).double()
        optimizer.step()
    return param.detach().numpy()


def own_error(tables, be, case, kind, native, steps=2):
    hp = ADAM_HP if kind == "adam" else SGD_HP
    net, _, start, grads = steps_with_record(tables, be, case, kind, native, steps, check_bits=native)
    mask = optim_cases.live_mask(net.num_params, optim.live_spans(net))
    exact = binary64_run(kind, hp, start, grads)
    return float(numpy.abs(host(net.flat_weights()).astype(numpy.float64) - exact)[mask].max())


def check_two_steps(be, kind, report=print):
    """b5_k4_stacked, two ``update_weights`` steps: the restatement bit for bit, torch within the yardstick."""
    mine = own_error(fc_train_cases, be, FC_CASE, kind, True)
    theirs = own_error(fc_train_cases, be, FC_CASE, kind, False)
    report(f"{kind} on {FC_CASE['name']}: native error {mine:.3e} against binary64, torch float32's own {theirs:.3e} "
           f"({mine / theirs if theirs else float('inf'):.2f} x; gate 4 x)")
    assert theirs > 0 and mine <= 4 * theirs


def check_residual(be, kind):
    """A residual network, weight decay on: the parameters are the restatement's, the statistics spans hold exactly what
    the step committed, and the optimizer state over them is exactly zero."""
    tables, case = resnet_train_cases, RESNET_CASE
    net, optimizer, start, _ = steps_with_record(tables, be, case, kind, True, 1, check_bits=True)
    committed = tables.run_native(be, case, tables.network(be, case))
    flat = host(net.flat_weights())
    s1, s2 = state_arrays(optimizer, kind, net.num_params)
    seen = 0
    for key, off, numel, shape in net._tensors:
        if common.is_statistic(key):
            seen += 1
            assert numpy.array_equal(optim_cases.bits(flat[off:off + numel]), optim_cases.bits(committed["stat/" + key])), key
            for s in (s1, s2):
                assert s is None or not optim_cases.bits(s[off:off + numel]).any(), key      # exact +0.0
        else:
            assert (flat[off:off + numel] != start[off:off + numel]).any(), key
    assert seen > 0


def check_stem(be, case, kind):
    """Behind a downsample stem the bypassed conv / bn tensors keep their bits through a step with weight decay, and
    their state is exactly zero; so is the state over every statistic."""
    tables = resnet_stem_train_cases
    net, optimizer, start, _ = steps_with_record(tables, be, case, kind, True, 1, check_bits=True)
    flat = host(net.flat_weights())
    s1, s2 = state_arrays(optimizer, kind, net.num_params)
    seen = 0
    for key, off, numel, shape in net._tensors:
        if tables.is_bypassed(key):
            seen += 1
            assert not key.endswith("conv.weight") or numpy.abs(start[off:off + numel]).max() > 0      # decay would move it
            assert numpy.array_equal(optim_cases.bits(flat[off:off + numel]), optim_cases.bits(start[off:off + numel])), key
        if tables.is_bypassed(key) or common.is_statistic(key):
            for s in (s1, s2):
                assert s is None or not optim_cases.bits(s[off:off + numel]).any(), key
    assert seen >= 4      # conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var


def check_round_trip(be, kind):
    common.check_optimizer_state_round_trip(be, fc_train_cases, FC_CASE, make(kind, True), lambda net: net._tensors)


def check_reference_state_loads(be, kind, report=print):
    """Two steps with the torch optimizer, its state saved in the reference's per-parameter format; a second network takes
    the weights, a NATIVE optimizer takes the state; the third step of both, from the same bits, agrees within the
    yardstick."""
    tables, case = fc_train_cases, FC_CASE
    hp = ADAM_HP if kind == "adam" else SGD_HP
    net, theirs, _, _ = steps_with_record(tables, be, case, kind, False, 2)
    saved = trainer.optimizer_state(theirs, net)
    twin = tables.network(be, case)
    twin.set_weights(net.get_weights())
    mine = make(kind, True)(twin.parameters())
    trainer.load_optimizer_state(mine, twin, saved)
    n = net.num_params
    start = host(net.flat_weights())
    assert numpy.array_equal(optim_cases.bits(start), optim_cases.bits(host(twin.flat_weights())))
    state = state_arrays(theirs, kind, n)
    for a, b in zip(state, state_arrays(mine, kind, n)):
        assert a is None or numpy.array_equal(optim_cases.bits(a), optim_cases.bits(b))
    for model, optimizer in ((net, theirs), (twin, mine)):
        trainer.update_weights(model, optimizer, tables.batch(case), tables.config_of(case))
    grad = host(next(net.parameters()).grad)
    assert numpy.array_equal(optim_cases.bits(grad), optim_cases.bits(host(next(twin.parameters()).grad)))
    if kind == "adam":
        assert float(mine.state_dict()["state"][0]["step"]) == 3.0
    exact = binary64_run(kind, hp, start, [grad], state=state, first_t=3)
    err_theirs = float(numpy.abs(host(net.flat_weights()) - exact).max())
    err_mine = float(numpy.abs(host(twin.flat_weights()) - exact).max())
    report(f"{kind}, third step from a loaded reference-format state: native error {err_mine:.3e}, torch float32's own {err_theirs:.3e}")
    assert err_theirs > 0 and err_mine <= 4 * err_theirs
    want = restated_step(kind, hp, 3, start, grad, state[0], state[1])[0]
    assert numpy.array_equal(optim_cases.bits(host(twin.flat_weights())), optim_cases.bits(want))


def check_constructor_refusals(be):
    net = fc_train_cases.network(be, FC_CASE)
    other = fc_train_cases.network(be, FC_CASE)
    for name, value in (("amsgrad", True), ("maximize", True), ("capturable", True), ("fused", False), ("fused", True),
                        ("foreach", False), ("foreach", True), ("differentiable", True)):
        with pytest.raises(NotImplementedError, match=name):
            optim.Adam(net.parameters(), lr=0.01, **{name: value})
    for name, value in (("nesterov", True), ("dampening", 0.1), ("maximize", True), ("foreach", True), ("fused", True),
                        ("differentiable", True)):
        with pytest.raises(NotImplementedError, match=name):
            optim.SGD(net.parameters(), lr=0.01, momentum=0.9, **{name: value})
    for cls in (optim.Adam, optim.SGD):
        with pytest.raises(NotImplementedError, match="param group"):
            cls([dict(params=list(net.parameters())), dict(params=list(other.parameters()))], lr=0.01)
        with pytest.raises(ValueError, match="flat parameter"):
            cls([torch.nn.Parameter(torch.zeros(4))], lr=0.01)
        with pytest.raises(ValueError, match="flat parameter"):
            cls([torch.nn.Parameter(net.flat_weights())], lr=0.01)      # the same storage, not the network's leaf
        assert cls(net, lr=0.01).param_groups[0]["params"][0] is next(net.parameters())      # the network itself
        assert cls([dict(params=list(net.parameters()))], lr=0.01).param_groups[0]["lr"] == 0.01
    config = fc_train_cases.config_of(FC_CASE, optimizer="Adam", lr_init=0.003, weight_decay=2e-4, momentum=0.8)
    adam = optim.from_config(net, config)
    assert isinstance(adam, optim.Adam) and isinstance(adam, torch.optim.Adam)
    assert adam.param_groups[0]["lr"] == 0.003 and adam.param_groups[0]["weight_decay"] == 2e-4
    config.optimizer = "SGD"
    sgd = optim.from_config(net, config)
    assert isinstance(sgd, optim.SGD) and isinstance(sgd, torch.optim.SGD)
    assert sgd.param_groups[0]["momentum"] == 0.8 and sgd.param_groups[0]["weight_decay"] == 2e-4
    config.optimizer = "RMSprop"
    with pytest.raises(NotImplementedError, match="RMSprop is not implemented. You can change the optimizer manually in trainer.py."):
        optim.from_config(net, config)
