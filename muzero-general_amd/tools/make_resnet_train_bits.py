"""
Writes one backend's section of tests/golden/resnet_train_bits.json: a SHA-256 of the bits of every output of
mzx_train_resnet_step -- the four losses, the priorities, the three logits, the whole gradient buffer and the packed running
statistics -- for the ten fixture cases of tests/resnet_train_cases.py and tests/resnet_stem_train_cases.py, together with
the commit it ran at.

    python muzero-general_amd/tools/make_resnet_train_bits.py --backend serial|device [--commit ID] [--out FILE]

The fixture pins what a change that must not move any sum has to reproduce, so it is recorded at the commit BEFORE such a
change (a checkout of that commit with this file copied in), the serial section on the host and the device section on an
MI355X, never at the code under test.  tests/test_resnet_train_bits.py and tests/test_gpu_resnet_train_bits.py compare
against it.  --commit names the commit where the tree carries no git metadata.
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
PINNED = ("loss", "value_loss", "reward_loss", "policy_loss", "priorities", "value_logits", "reward_logits", "policy_logits",
          "grad_flat", "running")
FIXTURE = os.path.join(ROOT, "tests", "golden", "resnet_train_bits.json")


def fixture_cases():
    """[(case, its tables module)] in the order of the fixture."""
    import resnet_stem_train_cases
    import resnet_train_cases
    return [(resnet_train_cases.BY_NAME[n], resnet_train_cases) for n in PLAIN] + \
           [(resnet_stem_train_cases.BY_NAME[n], resnet_stem_train_cases) for n in STEM]


def digests(got):
    """output -> SHA-256 of its float32 bits (shape and order as ``run_native`` returns them)."""
    out = {}
    for key in PINNED:
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
    ap.add_argument("--backend", choices=("serial", "device"), required=True)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], check=True, capture_output=True,
                                           text=True).stdout.strip()
    be = backend(args.backend)
    section = {"commit": commit, "cases": {}}
    for case, tables in fixture_cases():
        section["cases"][case["name"]] = digests(tables.run_native(be, case))
        print(case["name"], section["cases"][case["name"]]["grad_flat"][:16], flush=True)
    whole = {}
    if os.path.isfile(args.out):
        with open(args.out) as f:
            whole = json.load(f)
    whole[args.backend] = section
    with open(args.out, "w") as f:
        json.dump(whole, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote the {args.backend} section of {args.out} at {commit}")


if __name__ == "__main__":
    main()
