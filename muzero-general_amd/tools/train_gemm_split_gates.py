"""
How much of each reference gate the split-BF16 tiled GEMMs use, next to the wave route in the same run: per case of
tests/test_gpu_train_gemm_split.py the largest error / gate over every gated figure that resnet_train_cases.check_case /
check_live report (logits, losses, every gradient and statistic tensor), for a default handle and for one with
train_gemm = "tiled_all", train_matrix = "bf16x3".  Nothing is asserted here (the test does that); a case whose check raised
says so.

    python muzero-general_amd/tools/train_gemm_split_gates.py [--out profiles/train_gemm_split_gpu.log]
"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "muzero-general_amd"), os.path.join(ROOT, "tests")]
FIGURE = re.compile(r"^\S+ (.*?): error ([0-9.e+-]+).*gate ([0-9.e+-]+)")


def fractions(be, module, case, tables, live):
    import resnet_train_cases as plain

    worst, failed = [0.0, None], None

    def report(text):
        found = FIGURE.match(text)
        if found and float(found.group(2)) / float(found.group(3)) > worst[0]:
            worst[:] = [float(found.group(2)) / float(found.group(3)), found.group(1)]
    try:
        if live:
            plain.check_live(be, case, report=report, tables=tables)
        else:
            plain.check_case(be, case, module.golden(os.path.join(ROOT, "tests", "golden")), report=report, tables=tables)
    except AssertionError as error:
        failed = str(error)[:200]
    return dict(fraction=round(worst[0], 4), on=worst[1], **({"check_raised": failed} if failed else {}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_gemm_split_gpu.log"))
    args = ap.parse_args()
    import torch

    from mzx import _lib
    from test_gpu_train_gemm_tiled import CASES, WIDE72
    from test_train_gemm_split import split_tables

    be = _lib.default_backend()
    lines = [f"# train_gemm_split_gpu: {torch.cuda.get_device_name(0)}; per case the largest error / gate over the figures check_case / "
             "check_live gate (references: the committed binary64 goldens, wide72 live in binary64), wave = a default handle, "
             "bf16x3 = train_gemm 'tiled_all' + train_matrix 'bf16x3', same process"]
    for module, case in CASES:
        line = dict(case=case["name"], wave=fractions(be, module, case, module, case is WIDE72),
                    bf16x3=fractions(be, module, case, split_tables(module), case is WIDE72))
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
        with open(args.out, "w") as log:
            log.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
