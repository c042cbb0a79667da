"""
Writes one backend's section of a training step's bit fixture: a SHA-256 of the bits of every output of the step -- the four
losses, the priorities, the three logits, the whole gradient buffer and, for a residual network, the packed running
statistics -- for the fixture cases of the family, together with the commit it ran at.

    python muzero-general_amd/tools/make_resnet_train_bits.py [--family resnet|fc] --backend serial|device [--commit ID] [--out FILE]

  resnet  mzx_train_resnet_step, the ten cases of tests/resnet_train_cases.py and tests/resnet_stem_train_cases.py
          -> tests/golden/resnet_train_bits.json
  fc      mzx_train_fc_step, the five cases of tests/fc_train_cases.py -> tests/golden/fc_train_bits.json

A fixture pins what a change that must not move any sum has to reproduce, so it is recorded at the commit BEFORE such a
change (a checkout of that commit with this file copied in), the serial section on the host and the device section on an
MI355X, never at the code under test.  tests/test_{fc,resnet}_train_bits.py and tests/test_gpu_{fc,resnet}_train_bits.py
compare against it.  --commit names the commit where the tree carries no git metadata.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "muzero-general_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PLAIN = ("a_b2_k1", "b_b3_k3", "c_b5_k4_stacked", "d_b70_k3", "e_b3_k3_dead")
STEM = ("sa_b2_k1", "sb_b3_k3", "sc_b5_k2_stacked", "ca_b2_k2", "cb_b3_k3_stacked")
FC = ("b1_k1_nolayers", "b3_k3_enc1", "b5_k4_stacked", "b130_k11_cartpole", "b2_k2_wide")
PINNED = ("loss", "value_loss", "reward_loss", "policy_loss", "priorities", "value_logits", "reward_logits", "policy_logits",
          "grad_flat", "running")
FIXTURE = os.path.join(ROOT, "tests", "golden", "resnet_train_bits.json")
# per family: the pinned outputs (a fully connected network has no running statistics) and the fixture file
FAMILIES = {"resnet": dict(pinned=PINNED, fixture=FIXTURE),
            "fc": dict(pinned=PINNED[:-1], fixture=os.path.join(ROOT, "tests", "golden", "fc_train_bits.json"))}


def fixture_cases(family="resnet"):
    """[(case, its tables module)] in the order of the family's fixture."""
    if family == "fc":
        import fc_train_cases
        return [(fc_train_cases.BY_NAME[n], fc_train_cases) for n in FC]
    import resnet_stem_train_cases
    import resnet_train_cases
    return [(resnet_train_cases.BY_NAME[n], resnet_train_cases) for n in PLAIN] + \
           [(resnet_stem_train_cases.BY_NAME[n], resnet_stem_train_cases) for n in STEM]


def digests(got, family="resnet"):
    """output -> SHA-256 of its float32 bits (shape and order as ``run_native`` returns them)."""
    out = {}
    for key in FAMILIES[family]["pinned"]:
        a = numpy.ascontiguousarray(got[key])
        assert a.dtype == numpy.float32, (key, a.dtype)
        out[key] = hashlib.sha256(a.tobytes()).hexdigest()
    return out


def backend(name):
    if name == "serial":
        import hostcheck
        return hostcheck.backend()
    from mzx import _lib
    return _lib.default_backend()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=sorted(FAMILIES), default="resnet")
    ap.add_argument("--backend", choices=("serial", "device"), required=True)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or FAMILIES[args.family]["fixture"]
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], check=True, capture_output=True,
                                           text=True).stdout.strip()
    be = backend(args.backend)
    section = {"commit": commit, "cases": {}}
    for case, tables in fixture_cases(args.family):
        section["cases"][case["name"]] = digests(tables.run_native(be, case), args.family)
        print(case["name"], section["cases"][case["name"]]["grad_flat"][:16], flush=True)
    whole = {}
    if os.path.isfile(out_path):
        with open(out_path) as f:
            whole = json.load(f)
    whole[args.backend] = section
    with open(out_path, "w") as f:
        json.dump(whole, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote the {args.backend} section of {out_path} at {commit}")


if __name__ == "__main__":
    main()
