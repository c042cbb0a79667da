"""
The piece lifetime of the device hand-off under the address and undefined-behaviour sanitizers: tests/handoff_asan_main.cpp,
a stand-alone program with its own main that includes the library source as the serial build (-DMZX_HOSTCHECK), plays two
hand-off groups over many chunk ends, takes the pieces, ingests them into a small pool from the pieces' own arrays, exports
games again, releases, harvests into the released buffers and destroys the actors with pieces outstanding.  Recycling, a
stale token and destroy-with-pieces are where a host bug would turn into a GPU fault: they are walked here first.  Nothing is
loaded into the interpreter: the program is compiled with g++ -fsanitize=address,undefined (which links both runtimes) and
run as a child process.  CPU only.
"""
import os
import subprocess

from conftest import ROOT


def test_piece_lifetime_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "handoff_asan")
    src = os.path.join(ROOT, "tests", "handoff_asan_main.cpp")
    subprocess.run(["g++", "-O0", "-g1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DMZX_HOSTCHECK", "-x", "c++", src, "-o", exe],
                   check=True)
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert done.stdout.strip().endswith("ok") and "runtime error" not in done.stdout, done.stdout[-4000:]
