"""DevBuf (csrc/anm_devbuf.hpp), the owner of every device table of the C ABI layer, on the host: a stand-alone program
(tests/hostsim/devbuf_check.cpp; nothing here is loaded into Python) whose HIP calls are malloc / free / memcpy, plain
and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from gym_anm_amd import codegen

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "hostsim", "_build")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def build_program(sanitize):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "devbuf_check" + ("_san" if sanitize else ""))
    src = os.path.join(HERE, "hostsim", "devbuf_check.cpp")
    deps = [src, os.path.join(codegen.CSRC, "anm_devbuf.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        res = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall"] + (SANITIZE if sanitize else []) + [src, "-o", exe],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
    return exe


def run_program(exe):
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert "devbuf ok" in res.stdout and "none live" in res.stdout


def test_devbuf_owns_moves_and_frees():
    run_program(build_program(False))


def test_devbuf_under_the_address_and_undefined_behaviour_sanitizers():
    probe = os.path.join(OUT, "san_probe")
    os.makedirs(OUT, exist_ok=True)
    res = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                         capture_output=True, text=True)
    if res.returncode != 0 or subprocess.run([probe]).returncode != 0:
        pytest.skip("this g++ has no address / undefined-behaviour sanitizer runtime")
    run_program(build_program(True))
