"""
The workspace carve of mzx_train_chain under the address and undefined-behaviour sanitizers: tests/train_chain_asan_main.cpp,
a stand-alone program with its own main that includes the library source as the serial build (-DMZX_HOSTCHECK), gives the
chain heap blocks of exactly the sizes include/mzx.h asks for -- the workspace, the pool and sampler columns, the optimizer
state, the chunk table -- and runs three chained steps of a fully connected and of a residual network, with and without
PER, with Adam and with SGD.  A block carved short, or a launch that runs past its block, is a report here before it can
be a GPU fault.  Nothing is loaded into the interpreter: the program is compiled with g++ -fsanitize=address,undefined
(which links both runtimes) and run as a child process.  CPU only.
"""
import os
import subprocess

from conftest import ROOT


def test_chain_workspace_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "train_chain_asan")
    src = os.path.join(ROOT, "tests", "train_chain_asan_main.cpp")
    subprocess.run(["g++", "-O0", "-g1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DMZX_HOSTCHECK", "-x", "c++", src, "-o", exe],
                   check=True)
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert done.stdout.strip().endswith("ok") and "runtime error" not in done.stdout, done.stdout[-4000:]
