"""
Writes tests/golden/resnet_stem_train.npz: what the UNMODIFIED reference computes in one training step of a residual
network WITH a downsample stem ("resnet": DownSample, "CNN": DownsampleCNN) -- Trainer.update_weights on
models.MuZeroNetwork(config) in .train() mode on the CPU -- for the cases of tests/resnet_stem_train_cases.py.

    python muzero-general_amd/tools/make_resnet_stem_train_golden.py

Needs the reference checkout (oracle.ref_shim).  The layout of the file and the way the reference is run are those of
make_resnet_train_golden.py (its Recorder, its float32 and binary64 steps, its state-normalisation tie check are imported):
per case `<name>/digest`, `f32_*` (losses, step-major logits, decoded values), `f64_*` (losses, `f64_tensors`),
`f32_errors` per tensor and, for the case with an `sgd` entry, `f64_sgd_delta`; `keys` is a JSON object
{case: [state_dict keys in order]}.  Only arrays and that JSON go into the file; tensors are joined per case.

On top of the state-normalisation assertions the recipe asserts what the tie rules of the pooling kernels rest on, and
prints the counts:
  * in each CNN case at least one window of the first MaxPool2d has its maximum taken more than once (ReLU outputs tie
    at 0.0), so "the gradient goes to the first maximum in row-major window order" is exercised;
  * no window of either MaxPool2d holds two UNEQUAL values within 1e-6 of its maximum, so the reference's gradients do not
    depend on how rounding breaks a near-tie.
A seed that does not satisfy them is changed in the case table; the assertions stay.
"""
import json
import os
import sys

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "muzero-general_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_resnet_train_golden as plain  # noqa: E402
import resnet_stem_train_cases as cases  # noqa: E402
from oracle import ref_shim  # noqa: E402


def reference_model(ref_models, case, dtype):
    model = ref_models.MuZeroNetwork(cases.config_of(case))
    keys = [k for k in model.state_dict().keys() if not k.endswith("num_batches_tracked")]
    assert keys == list(cases.tensor_shapes(case)), (keys, list(cases.tensor_shapes(case)))
    state = {k: torch.from_numpy(v) for k, v in cases.weights(case).items()}
    for k in model.state_dict():
        if k.endswith("num_batches_tracked"):
            state[k] = torch.zeros((), dtype=torch.int64)
    model.set_weights(state)
    board = tuple(model.initial_inference(torch.zeros((2,) + cases.batch(case)[0].shape[1:]))[3].shape[2:])
    assert board == cases.hidden_board(case), (board, cases.hidden_board(case))
    model.set_weights(state)      # (the probe above moved the running statistics)
    return model.to(dtype).train(), keys


def watch_max_pools(model, windows):
    """(input, kernel, stride) of every MaxPool2d application, through forward pre-hooks."""
    for module in model.modules():
        if isinstance(module, torch.nn.MaxPool2d):
            module.register_forward_pre_hook(lambda m, i: windows.append(i[0].detach().clone()))


def check_pool_ties(case, pool_inputs):
    """-> (tied windows of the first pool, windows of the first pool)."""
    if case["stem"] != "CNN":
        assert not pool_inputs
        return 0, 0
    assert len(pool_inputs) == 2
    counts = []
    for x in pool_inputs:
        w = torch.nn.functional.unfold(x.double().flatten(0, 1).unsqueeze(1), kernel_size=3, stride=2)      # [planes, 9, windows]
        top = w.max(1, keepdim=True)[0]
        near = (w != top) & (top - w < 1e-6)
        assert not near.any(), (case["name"], "a near-tie of a pooling window's maximum")
        counts.append((int(((w == top).sum(1) > 1).sum()), int(w.shape[0] * w.shape[2])))
    assert counts[0][0] >= 1, (case["name"], "no window of the first pool has its maximum more than once: change the seed")
    return counts[0]


def main():
    ref_models, _ = ref_shim.load()
    import trainer as ref_trainer  # the reference's trainer.py, under the shim's ray stub

    plain.cases = cases      # the imported steps read the case tables (config_of, batch) of this module
    out, names = {}, {}
    for case in cases.CASES:
        name = case["name"]
        out[f"{name}/digest"] = numpy.array(cases.digest(case))
        results = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            model, keys = reference_model(ref_models, case, dtype)
            names[name] = keys
            states, pool_inputs = [], []
            plain.watch_states(model, states)
            watch_max_pools(model, pool_inputs)
            rec, losses = plain.one_step(ref_trainer, ref_models, case, dtype, model, plain.NoOptimizer())
            plain.check_ties(case, states)
            tied, total = check_pool_ties(case, pool_inputs)
            if tag == "f32":
                print(f"{name}: first max pool, {tied} tied windows of {total}; hidden board {cases.hidden_board(case)}")
            results[tag] = plain.tensors_after(model, keys)
            for key, value in zip(cases.LOSS_KEYS, losses):
                out[f"{name}/{tag}_{key}"] = numpy.asarray(value, numpy.float32 if tag == "f32" else numpy.float64)
            if tag == "f32":
                stack = lambda k: numpy.stack([s[k].detach().numpy() for s in rec.steps]).astype(numpy.float32)
                out[f"{name}/f32_value_logits"], out[f"{name}/f32_reward_logits"], out[f"{name}/f32_policy_logits"] = stack(0), stack(1), stack(2)
                out[f"{name}/f32_pred"] = numpy.stack([ref_models.support_to_scalar(s[0].detach(), case["S"]).numpy().squeeze(-1)
                                                       for s in rec.steps], 1).astype(numpy.float32)
        ordered = [("stat/" if cases.is_statistic(k) else "grad/") + k for k in keys]
        out[f"{name}/f64_tensors"] = numpy.concatenate([results["f64"][k].astype(numpy.float64).reshape(-1) for k in ordered])
        out[f"{name}/f32_errors"] = numpy.array([numpy.max(numpy.abs(results["f32"][k].astype(numpy.float64) - results["f64"][k]))
                                                 for k in ordered], numpy.float64)
        for key in keys:      # the bypassed tensors: no gradient, statistics untouched
            if cases.is_bypassed(key):
                kind = "stat/" if cases.is_statistic(key) else "grad/"
                want = cases.weights(case)[key] if cases.is_statistic(key) else 0.0
                assert numpy.array_equal(results["f32"][kind + key], numpy.broadcast_to(want, results["f32"][kind + key].shape)), key
        if "sgd" in case:
            model, keys = reference_model(ref_models, case, torch.float64)
            optimizer = torch.optim.SGD(model.parameters(), lr=case["sgd"]["lr"], momentum=case["sgd"]["momentum"],
                                        weight_decay=case["sgd"]["weight_decay"])
            for _ in range(2):
                plain.one_step(ref_trainer, ref_models, case, torch.float64, model, optimizer)
            initial = cases.weights(case)
            state = model.state_dict()
            for key, value in state.items():
                if key.endswith("num_batches_tracked"):
                    assert int(value) == cases.tracked_after(key, case, 2), (key, int(value))
            out[f"{name}/f64_sgd_delta"] = numpy.concatenate(
                [(state[key].detach().numpy() - initial[key].astype(numpy.float64)).astype(numpy.float32).reshape(-1) for key in keys])
        finite = [k for k, v in out.items() if k.startswith(name) and v.dtype.kind == "f" and not k.endswith("reward_logits")]
        assert all(numpy.isfinite(out[k]).all() for k in finite), case
    out["keys"] = numpy.array(json.dumps(names))
    path = os.path.join(ROOT, "tests", "golden", "resnet_stem_train.npz")
    numpy.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
